"""The read summary and MAPQ (scrg_read_summary, scrg_ctx_set_read_summary) on one box.  Prints one JSON line; --out FILE updates
that file under the part's key.

    --part kernels (default): device tensors, drawn distances and statuses, no alignment: the summary launch (with and without the
        statuses' copy) next to scrg_select_best's two launches in one loop, medians of alternating launches, on 1 M reads x 4
        candidates, 25 k x 4 and 1 000 reads x 4 000 candidates (which the wavefront form serves), with the bytes each must move.
    --part host: 1 M x 150 bp reads x 4 candidates against a resident genome, best-candidate mode: the setting off and on (the
        library's wall time, the added bytes down), and with the pileup on min_keep_q 0 and 20 (wall time, n_alignments).
    --part guard --base-lib LIB [--base-first]: the setting-off call of this library and of another build (the parent commit's),
        two handles in one process, interleaved; the parent's own call-to-call spread is the yardstick.

    python tests/tools/bench_mapq.py [--part kernels|host|guard] [--rounds 20] [--reads 1000000] [--passes 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def kernels_part(args):
    import torch
    import scrooge_amd
    from scrooge_amd import api
    dev = torch.device("cuda", 0)
    a = scrooge_amd.Aligner(0)
    a.set_stream(0)
    out = {"rounds": args.rounds}
    for name, nr, k in (("1M_x_4", 1_000_000, 4), ("25k_x_4", 25_000, 4), ("1k_x_4000", 1_000, 4_000)):
        n = nr * k
        rng = np.random.Generator(np.random.PCG64(1))
        first = torch.arange(0, n + 1, k, dtype=torch.int64, device=dev)
        ed = torch.from_numpy(rng.integers(0, 12, n)).to(dev)
        key = torch.arange(n, dtype=torch.int32, device=dev) // k
        length = torch.full((n,), 150, dtype=torch.int32, device=dev)
        status0 = torch.from_numpy((rng.random(n) < 0.05).astype(np.int32) * 2).to(dev)
        status, runs = status0.clone(), torch.full((n,), 7, dtype=torch.int32, device=dev)
        records = torch.zeros(32 * nr, dtype=torch.uint8, device=dev)
        keep = torch.zeros(n, dtype=torch.int32, device=dev)
        rule = api.MapqRule(min_keep_q=20)
        forms = [("read_summary", lambda: a.read_summary(nr, n, first, length, ed, status, records)),
                 ("read_summary_keep", lambda: a.read_summary(nr, n, first, length, ed, status, records, keep, rule=rule)),
                 ("select_best", lambda: a.select_best(n, key, ed, status, runs))]
        times = {f: [] for f, _ in forms}
        for r in range(args.rounds + 2):
            for f, fn in forms[r % 3:] + forms[:r % 3]:
                status.copy_(status0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    times[f].append(e0.elapsed_time(e1))
        rec = records.cpu().numpy().view(api.read_summary_dtype())
        row = {"reads": nr, "candidates_per_read": k, "pairs": n, "kept_fraction": float(((rec["flags"] & 8) != 0).mean()),
               "mean_mapq": float(rec["mapq"].mean()),
               # 8 bytes of offsets and 4 of read length per read, 12 per pair (distance, status); 32 per read written; the copy: 4 more
               # read and 4 written per pair
               "bytes_read_summary": 12 * nr + 12 * n + 32 * nr, "bytes_read_summary_keep": 12 * nr + 16 * n + 32 * nr + 4 * n,
               "bytes_select_best": 2 * (16 * n) + 9 * n}
        for f, v in times.items():
            row[f + "_ms"] = stats(v)
        row["read_summary_over_select_best"] = row["read_summary_ms"]["median"] / row["select_best_ms"]["median"]
        row["read_summary_GBps"] = row["bytes_read_summary"] / row["read_summary_ms"]["median"] / 1e6
        out[name] = row
    a.close()
    return out


def make_aligner(path):
    import scrooge_amd
    from scrooge_amd import api
    if path is None:
        return scrooge_amd.Aligner(0)
    saved, saved_v, api._LIB = api._LIB, api.SCRG_ABI_VERSION, None
    os.environ["SCRG_LIB"] = path
    try:
        return scrooge_amd.Aligner(0)
    finally:
        del os.environ["SCRG_LIB"]
        api._LIB, api.SCRG_ABI_VERSION = saved, saved_v


def batch(args):
    from tests.tools.bench_best import workload_a
    genome, reads, cands = workload_a(args.reads, G=args.genome)
    nr, L = reads.shape
    co = np.arange(nr + 1, dtype=np.uint64) * np.uint64(cands.shape[1])
    return genome, reads, L, co, cands.reshape(-1).astype(np.uint64)


def host_part(args):
    from scrooge_amd import api
    genome, reads, L, co, cs = batch(args)
    nr = len(co) - 1
    a = make_aligner(None)
    a.set_genome_array(genome)
    out = {"reads": nr, "read_len": int(L), "candidates_per_read": 4, "genome": int(genome.size), "passes": args.passes}

    def call(mapq=None):
        arr = a.align_mapping_rows(None, reads, L, co, cs, best=True, **({"mapq": mapq} if mapq is not None else {}))
        return a.last_timing["total_ns"] / 1e6, arr
    forms = [("off", None), ("on", True)]
    base = call()[1]
    on = call(True)[1]
    assert all(np.array_equal(base[k], on[k]) for k in ("edit_distance", "status", "run_offset", "cigar_offset", "runs")) and base["cigar_text"] == on["cigar_text"]
    rec = on["read_summary"]
    out["mapq_histogram"] = {str(q): int(c) for q, c in zip(*np.unique(rec["mapq"], return_counts=True))}
    out["tied_fraction"] = float(((rec["flags"] & 2) != 0).mean())
    times = {f: [] for f, _ in forms}
    for r in range(args.passes):
        for f, m in forms if r % 2 else forms[::-1]:
            times[f].append(call(m)[0])
    for f, v in times.items():
        out[f + "_ms"] = stats(v)
        out[f + "_ms"]["all"] = [round(x, 3) for x in v]
    out["added_ms_median"] = out["on_ms"]["median"] - out["off_ms"]["median"]
    out["added_bytes_down"] = 32 * nr
    out["added_bytes_up"] = 8 * nr
    # the pileup with the filter off and on
    a.set_pileup()
    try:
        pile = {}
        for q in (0, 20):
            t = []
            for r in range(3):
                ms, _ = call(api.MapqRule(min_keep_q=q))
                taken = a.take_pileup()
                if r:
                    t.append(ms)
            pile["min_keep_q_%d" % q] = {"call_ms": stats(t), "n_alignments": taken["n_alignments"], "n_out_of_range": taken["n_out_of_range"]}
        out["pileup"] = pile
    finally:
        a.set_pileup(False)
    a.close()
    return out


def guard_part(args):
    genome, reads, L, co, cs = batch(args)
    order = ["parent", "this"] if args.base_first else ["this", "parent"]
    als = {k: make_aligner(args.base_lib if k == "parent" else None) for k in order}
    out = {"order": order, "reads": len(co) - 1, "passes": args.passes}
    for al in als.values():
        al.set_genome_array(genome)
        al.align_mapping_rows(None, reads, L, co, cs, best=True)
    times = {k: [] for k in als}
    for _ in range(args.passes):
        for k, al in als.items():
            al.align_mapping_rows(None, reads, L, co, cs, best=True)
            times[k].append(al.last_timing["total_ns"] / 1e6)
    for k, v in times.items():
        out[k + "_off_ms"] = stats(v)
        out[k + "_off_ms"]["all"] = [round(x, 3) for x in v]
    p, t = out["parent_off_ms"], out["this_off_ms"]
    out["this_over_parent_median"] = t["median"] / p["median"]
    out["this_median_within_parent_range"] = bool(p["min"] <= t["median"] <= p["max"])
    for al in als.values():
        al.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels", choices=["kernels", "host", "guard"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--base-first", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part == "guard" and not args.base_lib:
        ap.error("--part guard compares with --base-lib")
    result = {"kernels": kernels_part, "host": host_part, "guard": guard_part}[args.part](args)
    key = args.part + ("_base_first" if args.part == "guard" and args.base_first else "")
    print(json.dumps({key: result}))
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc[key] = result
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
