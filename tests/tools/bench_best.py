"""Best-candidate mode (SCRG_OUT_BEST) through the host path: the same seeded mapping batch against a resident genome with the
flag off and on, in one process, interleaved, the median of --passes calls after a warm-up call of each form:
wall time per call (the library's clock, scrg_result.total_ns), bytes device -> host per call (12 or 8 bytes of wire per pair
+ 2 bytes per run + the text bytes: what stage 2 of scrg_host.cpp reads back) and kernel_ns, for outputs runs+text / text /
runs.  Workloads: (A) 1 M x 150 bp reads x 4 candidates (true locus, two shifted, one random: tests/tools/bench_mapping.py's
generator), (B) 25 k x 10 kb ONT-like reads x 4 candidates (true locus and three random ones).
--base-lib: another build of the library (the parent commit's) — the flag-off calls of both, interleaved in the same
process, for the guard that the mode costs nothing when it is off.

    python3 tests/tools/bench_best.py --workload A [--scale 1.0] [--passes 3] [--out profiles/best_only.json] [--base-lib lib.so]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

import scrooge_amd
from scrooge_amd import api, synth


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def workload_a(n_reads, G=100_000_000, seed=42):
    """tests/tools/bench_mapping.py's generator: reads of 150 bp with ~1 % errors from random loci of one random chromosome."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gcodes = rng.integers(0, 4, G, dtype=np.uint8)
    starts = rng.integers(0, G - 400, n_reads)
    L = 150
    seg = gcodes[starts[:, None] + np.arange(L + 8)[None, :]]
    sub = rng.random((n_reads, L + 8)) < 0.009
    seg = np.where(sub, (seg + rng.integers(1, 4, seg.shape, dtype=np.uint8)) & 3, seg)
    reads = seg[:, :L].copy()
    for r in np.nonzero(rng.random(n_reads) < 0.075)[0]:
        p = int(rng.integers(1, L - 1)); reads[r, p:] = seg[r, p + 1:L + 1]
    for r in np.nonzero(rng.random(n_reads) < 0.075)[0]:
        p = int(rng.integers(1, L - 1)); reads[r, p + 1:] = reads[r, p:L - 1].copy(); reads[r, p] = rng.integers(0, 4)
    sh1 = np.maximum(0, starts - rng.integers(1, 4, n_reads)); sh2 = starts + rng.integers(1, 4, n_reads)
    cands = np.stack([starts, sh1, sh2, rng.integers(0, G - 10, n_reads)], axis=1)
    return synth.BASES[gcodes], synth.BASES[reads], cands


def workload_b(n_reads, L=10000, seed=43):
    """One chromosome of n_reads segments of 1.09 L bases; read r is segment r with ONT-like errors (10 %, 23:31:46, one
    vectorised pass of synth.mutate's rule over the whole chromosome), cut to L bases.  Candidates: its segment and three
    random loci."""
    rng = np.random.Generator(np.random.PCG64(seed))
    S = int(L * 1.09) // 32 * 32
    G = n_reads * S
    gcodes = rng.integers(0, 4, G, dtype=np.uint8)
    err, ratio = synth.PROFILES["ont"]
    r = np.asarray(ratio, dtype=np.float64) / sum(ratio)
    u = rng.random(G, dtype=np.float32)
    hit = u < err
    kind = np.zeros(G, dtype=np.int8)
    kind[hit] = 1 + np.searchsorted(np.cumsum(r), rng.random(int(hit.sum())), side="right").clip(0, 2)
    out = gcodes.copy()
    sub = kind == 1
    out[sub] = (out[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
    emit = np.ones(G, dtype=np.int64)
    emit[kind == 2] = 2
    emit[kind == 3] = 0
    pos = np.cumsum(emit) - emit
    res = np.empty(int(emit.sum()), dtype=np.uint8)
    ins, keep = kind == 2, emit > 0
    res[pos[ins]] = rng.integers(0, 4, int(ins.sum()), dtype=np.uint8)
    res[pos[keep] + (emit[keep] - 1)] = out[keep]
    starts = np.arange(n_reads, dtype=np.int64) * S
    first = pos[starts]
    assert np.all(np.diff(np.append(first, len(res))) >= L)
    reads = res[first[:, None] + np.arange(L)[None, :]]
    cands = np.concatenate([starts[:, None], rng.integers(0, G - 2 * L, (n_reads, 3))], axis=1)
    return synth.BASES[gcodes], synth.BASES[reads], cands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["A", "B"], required=True)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="JSON file to update (key: the workload, or 'guard_<workload>' with --base-lib)")
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--base-last", action="store_true", help="make the handle of --base-lib second (and call it second in every pass): "
                    "the two handles of one process do not get the same hardware queues, so the guard is taken in both orders")
    args = ap.parse_args()

    n_reads = int((1_000_000 if args.workload == "A" else 25_000) * args.scale)
    genome, reads, cands = (workload_a if args.workload == "A" else workload_b)(n_reads)
    nr, L = reads.shape
    co = np.arange(nr + 1, dtype=np.uint64) * np.uint64(cands.shape[1])
    cs = cands.reshape(-1).astype(np.uint64)
    n = int(co[nr])
    log("workload %s: %d reads x %d bp x %d candidates, genome %d Mbp" % (args.workload, nr, L, cands.shape[1], genome.size // 1000000))

    def make_aligner(path):
        # a second build of the library next to the in-tree one: the handle keeps the library it was made with
        if path is None:
            return scrooge_amd.Aligner(0)
        saved, api._LIB = api._LIB, None
        os.environ["SCRG_LIB"] = path
        try:
            return scrooge_amd.Aligner(0)
        finally:
            del os.environ["SCRG_LIB"]
            api._LIB = saved

    def call(al, outputs, best):
        kw = {"best": True} if best else {}
        arr = al.align_mapping_rows(None, reads, L, co, cs, outputs=outputs, **kw)
        tm = al.last_timing
        want_text = outputs != api.SCRG_OUT_RUNS
        d2h = (12 if want_text else 8) * n + 2 * int(arr["run_offset"][n]) + int(arr["cigar_offset"][n])
        return {"total_ms": tm["total_ns"] / 1e6, "kernel_ms": tm["kernel_ns"] / 1e6, "pack_ms": tm["pack_ns"] / 1e6, "d2h_bytes": d2h}, arr

    def summary(samples):
        tot = sorted(s["total_ms"] for s in samples)
        return {"total_ms_median": tot[len(tot) // 2], "total_ms_all": [round(s["total_ms"], 3) for s in samples],
                "kernel_ms_median": sorted(s["kernel_ms"] for s in samples)[len(samples) // 2],
                "pack_ms_median": sorted(s["pack_ms"] for s in samples)[len(samples) // 2], "d2h_bytes": samples[0]["d2h_bytes"]}

    result = {"reads": nr, "read_len": L, "candidates_per_read": int(cands.shape[1]), "pairs": n, "passes": args.passes}
    if args.base_lib:
        if args.base_last:
            als = {"this": make_aligner(None), "parent": make_aligner(args.base_lib)}
        else:
            als = {"parent": make_aligner(args.base_lib), "this": make_aligner(None)}
        result["order"] = list(als)
        for al in als.values():
            al.set_genome_array(genome)
            call(al, api.SCRG_OUT_ALL, False)                      # warm-up: buffers, result arrays
        samples = {k: [] for k in als}
        for _ in range(args.passes):
            for k, al in als.items():
                samples[k].append(call(al, api.SCRG_OUT_ALL, False)[0])
        for k in als:
            result[k] = summary(samples[k])
            result[k]["range_ms"] = [min(result[k]["total_ms_all"]), max(result[k]["total_ms_all"])]
        lo = max(result["parent"]["range_ms"][0], result["this"]["range_ms"][0])
        hi = min(result["parent"]["range_ms"][1], result["this"]["range_ms"][1])
        result["ranges_overlap"] = bool(lo <= hi)
        key = "guard_" + args.workload + ("_base_last" if args.base_last else "")
    else:
        al = make_aligner(None)
        al.set_genome_array(genome)
        forms = [(name, o, b) for name, o in (("runs+text", api.SCRG_OUT_ALL), ("text", api.SCRG_OUT_TEXT), ("runs", api.SCRG_OUT_RUNS)) for b in (False, True)]
        keep = {}
        for name, o, b in forms:                                   # warm-up, and the check that the mode changes nothing else
            keep[(name, b)] = call(al, o, b)[1]
        for name, o, _ in forms[::2]:
            off, on = keep[(name, False)], keep[(name, True)]
            win = api.best_per_read(off["edit_distance"], off["status"], co)["best_pair"]
            assert np.array_equal(off["edit_distance"], on["edit_distance"])
            assert np.array_equal(np.flatnonzero(on["status"] != api.SCRG_PAIR_NOT_BEST), win[win >= 0])
            w = win[win >= 0]
            if o != api.SCRG_OUT_TEXT:
                assert int(on["run_offset"][n]) == int(np.sum(off["run_offset"][w + 1] - off["run_offset"][w]))
            if o != api.SCRG_OUT_RUNS:
                assert int(on["cigar_offset"][n]) == int(np.sum(off["cigar_offset"][w + 1] - off["cigar_offset"][w])) + (n - len(w))
        del keep
        samples = {(name, b): [] for name, _, b in forms}
        for _ in range(args.passes):
            for name, o, b in forms:
                samples[(name, b)].append(call(al, o, b)[0])
        for name, _, _ in forms[::2]:
            off, on = summary(samples[(name, False)]), summary(samples[(name, True)])
            result[name] = {"all": off, "best": on, "speedup": off["total_ms_median"] / on["total_ms_median"],
                            "d2h_ratio": on["d2h_bytes"] / off["d2h_bytes"]}
            log("%s %-9s all %.2f ms / %.1f MB   best %.2f ms / %.1f MB   x%.2f" % (args.workload, name, off["total_ms_median"], off["d2h_bytes"] / 1e6,
                                                                                 on["total_ms_median"], on["d2h_bytes"] / 1e6, result[name]["speedup"]))
        key = args.workload
    print(json.dumps({key: result}))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc[key] = result
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
