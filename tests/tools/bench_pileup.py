"""The pileup (scrg_pileup_add / scrg_pileup_finish, pileup_kernels.hip) timed on one GPU, in one process.

kernels  single launches on device buffers, medians of --launches (9) launches, the forms ALTERNATING launch by launch so that they
         share the box's state:
             align        scrg_align_device (its own events: scrg_last_kernel_ms)
             compact      scrg_compact_runs
             pileup_add   scrg_pileup_add on the dense runs into a zeroed accumulator of the genome's length (the zeroing is outside
                          the timed region)
             report       scrg_report_device on the same dense runs
             clip         scrg_clip_device on the same dense runs, records only
             finish       scrg_pileup_finish in place for that genome length
         for 100 000 x 10 kb ONT-error candidates at 64/33 spread over 2048 stretches of a target of 23.5 M positions (every
         position is covered ~43 times, so the atomics contend as they would on a deep pileup);
         with the atomics the pass issues per pair, counted from the runs (edges of '=' and 'D' stretches, 'X' columns, insertion
         events), and the columns per pair, which is what one add per column would issue.
host     scrg_align_mapping_resident on the same candidates with the setting on (and one take at the end) and off on this library,
         and off on --base-lib, a library built from the parent commit (scripts/ab.sh build), alternating call by call: the off
         path is held against the parent's.  --base-first makes the parent's handle first.
guard    the two off forms alone in the loop: the call with the setting on allocates, reads back and releases 28 bytes per genome base
         on this library's handle only, which the calls next to it in the loop feel.

    python3 tests/tools/bench_pileup.py [--base-lib ab_libs/lib_parent.so] [--base-first] [--part kernels|host|guard|all] [--scale 1.0]
                                        [--launches 9] [--out profiles/pileup.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

import scrooge_amd
from scrooge_amd import synth
from tests.tools.bench_distance import DeviceBatch, log, make_aligner, med
from tests.tools.bench_report import summary, timed


def genome_batch(n, L, seed):
    """2048 distinct ONT-error pairs, their texts back to back as the genome; n candidates that repeat them in a seeded order
    -> (genome bytes, read rows [2048, L], every candidate's read row, every candidate's start)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    err, ratio = synth.PROFILES["ont"]
    base_n = min(n, 2048)
    pairs = [synth.make_pair(L, err, ratio, rng) for _ in range(base_n)]
    starts = np.concatenate([[0], np.cumsum([len(t) for t, _ in pairs])]).astype(np.uint64)
    genome = b"".join(synth.BASES[t].tobytes() for t, _ in pairs)
    rows = np.stack([synth.BASES[q] for _, q in pairs])
    pick = rng.integers(0, base_n, n)
    return genome, rows, pick, starts[pick]


def count_atomics(t, dense, off, n):
    """What pileup_add issues for these runs, counted apart from it (torch, on the device): per stretch of '=' or 'D' runs two edges,
    per 'X' column and per insertion event one add -> (atomics, columns)."""
    runs = int(off[-1])
    d = dense[:2 * runs].view(-1, 2)
    cnt, op = d[:, 0].to(t.int64), d[:, 1].to(t.int64)
    prev = t.roll(op, 1)
    prev[off[:n][off[:n] < runs]] = 0                                         # the first run of every pair has no run before it
    stretch = (op == ord("=")) | (op == ord("D"))
    opens = int((stretch & (prev != op)).sum())
    x_cols = int(cnt[op == ord("X")].sum())
    ins = int(((op == ord("I")) & (prev != ord("I"))).sum())
    columns = int(cnt[op != ord("I")].sum())
    return 2 * opens + x_cols + ins, columns


def kernels_part(al, n, L, launches, seed):
    b = DeviceBatch(al, n, L, seed)
    t = b.torch
    dev = b.ed.device
    al.set_stream(0)
    b.arena()
    kw = dict(W=64, O=33, text_stride_words=64, read_stride_words=64)
    skw = dict(text_stride_words=64, read_stride_words=64)
    al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
    t.cuda.synchronize()
    assert int(b.st.max()) == 0
    b.off[1:] = t.cumsum(b.nr.to(t.int64), 0)
    runs = int(b.off[-1])
    assert 2 * runs <= b.dense.numel()
    # where the candidates lie: 2048 stretches of the longest text's length side by side, the candidates spread over them
    text_len = b.desc[:, 1]
    slot = int(text_len.max())
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    start = t.from_numpy(rng.integers(0, min(n, 2048), n) * slot).to(dev)
    target_len = min(n, 2048) * slot
    acc = t.zeros(7 * (target_len + 1), dtype=t.int32, device=dev)
    oor = t.zeros(1, dtype=t.int32, device=dev)
    rec = t.zeros((n, 8), dtype=t.int32, device=dev)
    rep = t.zeros((n, 8), dtype=t.int32, device=dev)
    fail = t.zeros(1, dtype=t.int32, device=dev)
    forms = {
        "compact": lambda: al.compact_runs(b.n, b.desc, b.slices, b.nr, b.off, b.dense),
        "pileup_add": lambda: al.pileup_add(n, b.seq, b.desc, b.dense, b.off, 1, b.nr, b.st, start, target_len, acc, oor, **skw),
        "report": lambda: al.report_device(n, b.seq, b.desc, b.dense, b.off, 1, b.nr, b.ed, b.st, rep, fail, **skw),
        "clip": lambda: al.clip_device(n, b.dense, b.off, 1, b.nr, b.st, rec),
        "finish": lambda: al.pileup_finish(target_len, acc),
    }
    samples = {k: [] for k in ["align"] + list(forms)}
    for it in range(launches + 1):                 # (the first round warms up)
        al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
        t.cuda.synchronize()
        ms = {"align": al.last_kernel_ms()}
        for k, fn in forms.items():
            if k == "pileup_add":
                acc.zero_()
                t.cuda.synchronize()
            ms[k] = timed(t, fn)
        if it:
            for k, v in ms.items():
                samples[k].append(v)
    assert int(fail) == 0 and int(oor) == 0
    counts = acc.view(7, target_len + 1)
    atomics, columns = count_atomics(t, b.dense, b.off, n)
    assert int(counts[:6].to(t.int64).sum()) == columns, "the planes do not hold every column once"
    out = {"pairs": n, "read_len": L, "launches": launches, "runs": runs, "target_len": target_len, "accumulator_bytes": int(acc.numel()) * 4,
           "atomics_per_pair": atomics / n, "columns_per_pair": columns / n, "runs_per_pair": runs / n,
           "mean_depth": columns / target_len}
    for k, v in samples.items():
        out[k + "_ms_median"] = med(v)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
    out["pileup_add_atomics_per_s"] = atomics / (out["pileup_add_ms_median"] / 1e3)
    out["pileup_add_over_report"] = out["pileup_add_ms_median"] / out["report_ms_median"]
    out["pileup_add_over_align"] = out["pileup_add_ms_median"] / out["align_ms_median"]
    log("%d x %d: align %.3f ms, compact %.3f, pileup_add %.3f (%.0f atomics per pair for %.0f columns), report %.3f, clip %.3f; finish of %d positions %.3f" % (
        n, L, out["align_ms_median"], out["compact_ms_median"], out["pileup_add_ms_median"], out["atomics_per_pair"], out["columns_per_pair"],
        out["report_ms_median"], out["clip_ms_median"], target_len, out["finish_ms_median"]))
    return out


def host_part(als, n, L, passes, seed, off_only=False):
    genome, rows, pick, starts = genome_batch(n, L, seed)
    forms = [f for f in [("parent_off", "parent", False), ("this_off", "this", False), ("this_pileup", "this", True)] if f[1] in als and not (off_only and f[2])]
    co = np.arange(n + 1, dtype=np.uint64)
    read_rows = rows[pick]
    for al in als.values():
        al.set_genome(genome)

    def call(who, on):
        al = als[who]
        if on:
            al.set_pileup(True)
        try:
            al.align_mapping_rows(None, read_rows, L, co, starts)
            ms = al.last_timing["total_ns"] / 1e6
            if on:
                got = al.take_pileup()
                assert got["n_alignments"] == n and got["target_len"] == len(genome)
        finally:
            if on:
                al.set_pileup(False)
        return ms

    for _, who, on in forms:
        call(who, on)
    samples = {f: [] for f, _, _ in forms}
    for _ in range(passes):
        for f, who, on in forms:
            samples[f].append(call(who, on))
    out = {f: summary(v) for f, v in samples.items()}
    out.update(pairs=n, read_len=L, passes=passes, genome_len=len(genome))
    if "this_pileup" in out:
        out["this_pileup_over_this_off"] = out["this_pileup"]["total_ms_median"] / out["this_off"]["total_ms_median"]
    if "parent_off" in out:
        ratio = out["this_off"]["total_ms_median"] / out["parent_off"]["total_ms_median"]
        out["this_off_over_parent_off"] = ratio
        out["this_off_within_4_percent"] = bool(abs(ratio - 1.0) <= 0.04)
    log("host %d x %d: %s" % (n, L, ", ".join("%s %.2f ms" % (f, out[f]["total_ms_median"]) for f, _, _ in forms)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--base-first", action="store_true", help="make the handle of --base-lib before this library's")
    ap.add_argument("--part", default="all", choices=["kernels", "host", "guard", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent = make_aligner(args.base_lib) if args.base_lib and args.base_first else None
    scrooge_amd.build_library()
    this = scrooge_amd.Aligner(0)
    if args.base_lib and parent is None:
        parent = make_aligner(args.base_lib)
    out = {}
    n = max(64, int(100000 * args.scale))
    if args.part in ("kernels", "all"):
        out["kernels_100k_x_10kb"] = kernels_part(this, n, 10000, args.launches, 1)
    als = {"this": this}
    if parent is not None:
        als["parent"] = parent
    if args.part in ("host", "all"):
        out["align_mapping_100k_x_10kb" + ("_base_first" if args.base_first else "")] = host_part(als, n, 10000, args.launches, 3)
    if args.part == "guard":
        out["off_only_100k_x_10kb" + ("_base_first" if args.base_first else "")] = host_part(als, n, 10000, args.launches, 3, off_only=True)
    print(json.dumps(out, indent=1, sort_keys=True))
    if args.out:
        if os.path.exists(args.out):              # (a second run, the other handle order: both stay in the file)
            with open(args.out) as f:
                out = dict(json.load(f), **out)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
