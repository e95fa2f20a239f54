"""The pileup sites (scrg_ctx_take_pileup_sites; scrg_pileup_sites_mark / _write, site_kernels.hip) timed on one GPU, in one process,
on the batch of profiles/pileup.json: 100 000 x 10 kb ONT-error candidates on a genome of 23.6 M positions, ~43-fold coverage.

takes    per repetition and form: one scrg_align_mapping_resident with the pileup on (not timed), then ONE take, timed as the C call
         alone (wall clock around the library call; the binding's copy into numpy is outside) — the forms in an order that
         alternates repetition by repetition:
             take_pileup           scrg_ctx_take_pileup: the baseline, 28 bytes per genome base brought down
             sites_1_1_0           scrg_ctx_take_pileup_sites, every position where anything disagrees or is inserted
             sites_8_3_200         ... at depth >= 8, where 3 observations and a fifth of the depth disagree
             parent_take_pileup    scrg_ctx_take_pileup of --base-lib, a library built from the parent commit (scripts/ab.sh build):
                                   the full take must not have moved
         with the number of sites and the bytes each brings down.
kernels  on the counts of one full take put back on the device and the genome packed there: scrg_pileup_sites_mark (the mark and
         the scan launches) and scrg_pileup_sites_write per rule, single calls between events, medians of --launches, alternating
         with a device-to-device copy of the seven planes — the copy rate this box reaches at that size — and each pass against the
         bytes it must move.

    python3 tests/tools/bench_pileup_sites.py [--base-lib ab_libs/lib_parent.so] [--part takes|kernels|all] [--scale 1.0]
                                              [--reps 5] [--launches 9] [--out profiles/pileup_sites.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

import scrooge_amd
from scrooge_amd import api
from tests.tools.bench_distance import log, make_aligner, med
from tests.tools.bench_pileup import genome_batch
from tests.tools.bench_report import timed

RULES = {"sites_1_1_0": (1, 1, 0), "sites_8_3_200": (8, 3, 200)}


def summary(ms):
    return {"ms_median": med(ms), "ms_all": [round(x, 3) for x in ms], "range_ms": [min(ms), max(ms)]}


def take_full(al):
    """scrg_ctx_take_pileup, the C call alone -> (ms, bytes brought down, the counts)"""
    fn, free = api._lazy(al.lib, "scrg_ctx_take_pileup"), api._lazy(al.lib, "scrg_pileup_free")
    r = C.POINTER(api.Pileup)()
    t0 = time.perf_counter()
    st = fn(al.h, C.byref(r))
    ms = (time.perf_counter() - t0) * 1e3
    al._check(st)
    try:
        n = int(r.contents.target_len) + 1
        counts = np.ctypeslib.as_array(r.contents.counts, shape=(api.SCRG_PILE_PLANES * n,)).copy().reshape(api.SCRG_PILE_PLANES, n)
        return ms, 4 * api.SCRG_PILE_PLANES * n + 8, counts, int(r.contents.n_alignments)
    finally:
        free(r)


def take_sites(al, rule):
    """scrg_ctx_take_pileup_sites, the C call alone -> (ms, bytes brought down, n_sites)"""
    fn, free = api._lazy(al.lib, "scrg_ctx_take_pileup_sites"), api._lazy(al.lib, "scrg_pileup_sites_free")
    k = api.SiteRule(*rule, 0)
    r = C.POINTER(api.PileupSites)()
    t0 = time.perf_counter()
    st = fn(al.h, C.byref(k), C.byref(r))
    ms = (time.perf_counter() - t0) * 1e3
    al._check(st)
    try:
        n = int(r.contents.n_sites)
        return ms, 8 + 8 + 40 * n, n, int(r.contents.n_alignments)
    finally:
        free(r)


def takes_part(als, n, L, reps, seed):
    genome, rows, pick, starts = genome_batch(n, L, seed)
    co = np.arange(n + 1, dtype=np.uint64)
    read_rows = rows[pick]
    for al in als.values():
        al.set_genome(genome)
        al.set_pileup(True)
    forms = [("take_pileup", "this", None)] + [(f, "this", r) for f, r in RULES.items()]
    if "parent" in als:
        forms.append(("parent_take_pileup", "parent", None))
    samples = {f: [] for f, _, _ in forms}
    facts = {}
    counts = None
    try:
        for rep in range(reps + 1):                # (the first repetition warms up: allocations, the first launches)
            for f, who, rule in (forms if rep % 2 == 0 else forms[::-1]):
                al = als[who]
                al.align_mapping_rows(None, read_rows, L, co, starts)
                if rule is None:
                    ms, down, counts, n_aln = take_full(al)
                    facts[f] = {"bytes_down": down}
                else:
                    ms, down, n_sites, n_aln = take_sites(al, rule)
                    facts[f] = {"bytes_down": down, "n_sites": n_sites, "rule": list(rule)}
                assert n_aln == n
                if rep:
                    samples[f].append(ms)
    finally:
        for al in als.values():
            al.set_pileup(False)
    out = {f: dict(summary(v), **facts[f]) for f, v in samples.items()}
    # the sites the device found are the host twin's on the counts of the full take
    for f, rule in RULES.items():
        assert len(api.pileup_sites_from_counts(counts, genome, *rule)) == out[f]["n_sites"], f
    depth = counts[:6, :len(genome)].astype(np.int64).sum(axis=0)
    out.update(pairs=n, read_len=L, reps=reps, genome_len=len(genome), mean_depth=float(depth.mean()), covered=int((depth > 0).sum()))
    for f in RULES:
        out[f + "_over_take_pileup"] = out[f]["ms_median"] / out["take_pileup"]["ms_median"]
    if "parent_take_pileup" in out:
        out["take_pileup_over_parent"] = out["take_pileup"]["ms_median"] / out["parent_take_pileup"]["ms_median"]
    log("takes %d x %d on %d positions: %s" % (n, L, len(genome), ", ".join("%s %.2f ms (%d bytes down)" % (f, out[f]["ms_median"], out[f]["bytes_down"])
                                                                          for f, _, _ in forms)))
    return out, genome, counts


def kernels_part(al, genome, counts, launches):
    import torch as t
    dev = t.device("cuda", al.device)
    al.set_stream(0)
    L = len(genome)
    d_counts = t.from_numpy(counts.view(np.int32).reshape(-1)).to(dev)
    d_copy = t.empty_like(d_counts)
    flat = np.frombuffer(genome, dtype=np.uint8)
    flat = np.concatenate([flat, np.full((-L) % 32 + 32 * (api.SEQ_PAD_WORDS + 1), ord("A"), dtype=np.uint8)])
    seq = t.zeros(len(flat) // 32 + api.SEQ_PAD_WORDS, dtype=t.int64, device=dev)
    bad = t.zeros(1, dtype=t.int32, device=dev)
    al.pack_planar(t.from_numpy(flat).to(dev), seq, bad)
    assert int(bad) == 0
    scratch = t.empty(al.pileup_sites_scratch_bytes(L) // 8, dtype=t.int64, device=dev)
    n_dev = t.zeros(1, dtype=t.int64, device=dev)
    n_sites = {}
    for f, rule in RULES.items():
        al.pileup_sites_mark(L, d_counts, seq, 0, rule, scratch, n_dev)
        t.cuda.synchronize()
        n_sites[f] = int(n_dev[0])
    sites = t.empty(5 * max(max(n_sites.values()), 1), dtype=t.int64, device=dev)
    samples = {"copy_planes": []}
    for f in RULES:
        samples[f + "_mark_scan"] = []
        samples[f + "_write"] = []
    for it in range(launches + 1):                 # (the first round warms up)
        ms = {"copy_planes": timed(t, lambda: d_copy.copy_(d_counts))}
        for f, rule in RULES.items():
            ms[f + "_mark_scan"] = timed(t, lambda: al.pileup_sites_mark(L, d_counts, seq, 0, rule, scratch, n_dev))
            ms[f + "_write"] = timed(t, lambda: al.pileup_sites_write(L, d_counts, seq, 0, scratch, n_sites[f], sites))
        if it:
            for k, v in ms.items():
                samples[k].append(v)
    plane_bytes = 4 * 7 * (L + 1)
    out = {"target_len": L, "launches": launches, "plane_bytes": plane_bytes}
    for k, v in samples.items():
        out[k + "_ms_median"] = med(v)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
    out["copy_planes_GBps"] = 2 * plane_bytes / out["copy_planes_ms_median"] / 1e6            # read and write
    for f in RULES:
        # what each pass must move: mark reads the planes and the genome's 2 bits per base and writes one bit per position;
        # write reads the bitmap, 28 bytes and a genome word per site, and stores 40 bytes per site
        mark_bytes = plane_bytes + L // 4 + L // 8
        write_bytes = L // 8 + n_sites[f] * (28 + 8 + 40)
        out[f] = {"n_sites": n_sites[f], "mark_bytes": mark_bytes, "write_bytes": write_bytes,
                  "mark_scan_GBps": mark_bytes / out[f + "_mark_scan_ms_median"] / 1e6, "write_GBps": write_bytes / out[f + "_write_ms_median"] / 1e6}
        out[f]["mark_scan_over_copy_rate"] = out[f]["mark_scan_GBps"] / out["copy_planes_GBps"]
    log("kernels on %d positions: copy of the planes %.3f ms (%.0f GB/s); %s" % (
        L, out["copy_planes_ms_median"], out["copy_planes_GBps"],
        "; ".join("%s mark+scan %.3f ms (%.0f GB/s), write %.3f ms, %d sites" % (f, out[f + "_mark_scan_ms_median"], out[f]["mark_scan_GBps"], out[f + "_write_ms_median"],
                                                                          n_sites[f]) for f in RULES)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--part", default="all", choices=["takes", "kernels", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "ranges over at least three repetitions"
    scrooge_amd.build_library()
    this = scrooge_amd.Aligner(0)
    als = {"this": this}
    if args.base_lib:
        als["parent"] = make_aligner(args.base_lib)
    n = max(64, int(100000 * args.scale))
    out = {}
    takes, genome, counts = takes_part(als, n, 10000, args.reps, 3)
    if args.part in ("takes", "all"):
        out["takes_100k_x_10kb"] = takes
    if args.part in ("kernels", "all"):
        out["kernels_100k_x_10kb"] = kernels_part(this, genome, counts, args.launches)
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
