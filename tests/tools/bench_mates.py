"""Paired-end selection next to best-candidate selection, one loop on one box.  Prints one JSON line.

    --part kernels (default): device tensors, 500 k mate pairs x (4 + 4) candidates, drawn distances, starts and strands, no alignment:
        the selection launch alone with the team size given (scrg_select_mates_team: one launch, exact grid), scrg_select_mates (team
        pass, then the selection on a grid sized for teams of 64) and scrg_select_best's two launches on the same 4 M pairs.
    --part host: 1 M x 150 bp reads x 4 candidates against a resident genome (tests/tools/bench_mapping.py's shape on a smaller
        chromosome): scrg_align_mapping_paired next to scrg_align_mapping_resident | SCRG_OUT_BEST, the library's own wall time.
    --part best: the best-mode call of --part host alone (for a library named by SCRG_LIB: the parent commit's, which has no
        paired call), the same batch.

    python tests/tools/bench_mates.py [--part kernels|host|best] [--mates 500000] [--cands 4] [--rounds 20] [--reads 1000000]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def host_part(args):
    import scrooge_amd
    from scrooge_amd import api, synth
    rng = np.random.Generator(np.random.PCG64(42))
    G, L, nr = 20_000_000, 150, args.reads
    gcodes = rng.integers(0, 4, G, dtype=np.uint8)
    genome = synth.BASES[gcodes].tobytes()
    # mate pairs: A forward at s, B reverse 200 .. 500 further on; 1 % substitutions
    s_a = rng.integers(0, G - 1200, nr // 2)
    starts = np.stack([s_a, s_a + rng.integers(200, 500, nr // 2)], axis=1).ravel()
    seg = gcodes[starts[:, None] + np.arange(L)[None, :]]
    seg = np.where(rng.random(seg.shape) < 0.01, (seg + rng.integers(1, 4, seg.shape, dtype=np.uint8)) & 3, seg)
    is_rev = (np.arange(nr) % 2).astype(bool)
    seg[is_rev] = 3 - seg[is_rev][:, ::-1]
    ascii_reads = synth.BASES[seg]
    reads = [ascii_reads[r].tobytes() for r in range(nr)]
    cands = np.stack([starts, np.maximum(0, starts - rng.integers(1, 4, nr)), starts + rng.integers(1, 4, nr), rng.integers(0, G - 200, nr)], axis=1).tolist()
    rev = np.repeat(is_rev.astype(int)[:, None], 4, axis=1).tolist()
    a = scrooge_amd.Aligner(0)
    a.set_genome(genome)
    out = {"part": args.part, "reads": nr, "candidates_per_read": 4, "read_len": L, "genome": G, "library": "named by SCRG_LIB" if os.environ.get("SCRG_LIB") else "this"}

    def best():
        a.align_mapping_directed(reads, cands, reverse=rev, arrays=True, best=True)
        return a.last_timing["total_ns"] / 1e6

    def paired():
        _, mates = a.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(100, 1000, "fr", 2), arrays=True)
        out["proper_fraction"] = float((mates["flags"] & 1).mean())
        return a.last_timing["total_ns"] / 1e6
    forms = [("best_ms", best)] + ([("paired_ms", paired)] if args.part == "host" else [])
    times = {name: [] for name, _ in forms}
    for r in range(4):
        for name, fn in forms if r % 2 else forms[::-1]:
            v = fn()
            if r:
                times[name].append(v)
    for name, v in times.items():
        out[name] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(json.dumps(out))
    a.close()


def main():
    import torch
    import scrooge_amd
    from scrooge_amd import api
    ap = argparse.ArgumentParser()
    ap.add_argument("--mates", type=int, default=500000)
    ap.add_argument("--cands", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--part", default="kernels")
    ap.add_argument("--reads", type=int, default=1000000)
    args = ap.parse_args()
    if args.part != "kernels":
        return host_part(args)
    nm, k = args.mates, args.cands
    n = 2 * nm * k
    rng = np.random.Generator(np.random.PCG64(1))
    dev = torch.device("cuda", 0)
    a = scrooge_amd.Aligner(0)
    a.set_stream(0)
    locus = np.repeat(rng.integers(0, 3_000_000_000, nm), 2 * k)
    t = {"first": torch.arange(0, n + 1, k, dtype=torch.int64, device=dev),
         "start": torch.from_numpy(locus + rng.integers(0, 600, n)).to(dev),
         "len": torch.full((n,), 150, dtype=torch.int32, device=dev),
         "rev": torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).to(dev),
         "ed": torch.from_numpy(rng.integers(0, 12, n)).to(dev),
         "key": torch.arange(n, dtype=torch.int32, device=dev) // k}
    status0 = torch.zeros(n, dtype=torch.int32, device=dev)
    runs0 = torch.full((n,), 7, dtype=torch.int32, device=dev)
    status, runs = status0.clone(), runs0.clone()
    records = torch.zeros(32 * nm, dtype=torch.uint8, device=dev)
    rule = api.MateRule(100, 1000, "fr", 2)

    def mates():
        a.select_mates(nm, t["first"], t["start"], t["len"], t["rev"], t["ed"], status, runs, None, records, rule=rule)

    def mates_team():
        a.select_mates(nm, t["first"], t["start"], t["len"], t["rev"], t["ed"], status, runs, None, records, rule=rule, team=16 if k * k > 8 else 8 if k * k > 4 else 4)

    def best():
        a.select_best(n, t["key"], t["ed"], status, runs)
    forms = [("select_mates_team", mates_team), ("select_mates", mates), ("select_best", best)]
    times = {name: [] for name, _ in forms}
    for r in range(args.rounds + 2):
        for name, fn in forms[r % 3:] + forms[:r % 3]:
            status.copy_(status0)
            runs.copy_(runs0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append(e0.elapsed_time(e1))
    rec = records.cpu().numpy().view(api.mate_dtype())
    out = {"mates": nm, "candidates_per_read": k, "pairs": n, "rounds": args.rounds, "proper_fraction": float((rec["flags"] & 1).mean())}
    for name, v in times.items():
        out[name + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(json.dumps(out))
    a.close()


if __name__ == "__main__":
    main()
