"""The clip pass (scrg_clip_device, clip_kernels.hip) timed on one GPU, in one process.

kernels  single launches on device buffers, medians of --launches (9) launches, the forms ALTERNATING launch by launch so that they
         share the box's state:
             align        scrg_align_device (its own events: scrg_last_kernel_ms)
             compact      scrg_compact_runs
             clip         scrg_clip_device on the dense runs, records only
             clip_apply   scrg_clip_device on the slices and descriptors in apply mode, as stage 1 of the host path runs it (the pass
                          and its element-wise second launch; the descriptors are put back outside the timed region)
             report       scrg_report_device on the same dense runs: the pass this one is held against — it reads the same runs and
                          the sequences besides
         for 100 000 x 10 kb ONT-error pairs at 64/33; with the bytes the pass must read (runs, counts, offsets, status) and writes
         (32 per pair), and that traffic over the measured time as a fraction of the HBM roof (8 TB/s peak).
host     scrg_align_pairs on 100 000 x 10 kb pairs with the setting on and off on this library, and off on --base-lib, a library built
         from the parent commit (scripts/ab.sh build), alternating call by call: the off path is held against the parent's (ratio of
         the medians, and whether it lies within the +-4 % box-to-box spread the README states).  --base-first makes the parent's
         handle first (two handles of one process do not get equal treatment, tests/tools/bench_diff.py).

    python3 tests/tools/bench_clip.py [--base-lib ab_libs/lib_parent.so] [--base-first] [--part kernels|host|all] [--scale 1.0] [--launches 9]
                                      [--out profiles/clip.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

import scrooge_amd
from tests.tools.bench_distance import DeviceBatch, log, make_aligner, make_rows, med
from tests.tools.bench_report import HBM_PEAK, summary, timed


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
    desc0 = b.desc.clone()
    rec = t.zeros((n, 8), dtype=t.int32, device=dev)
    rec_apply = t.zeros((n, 8), dtype=t.int32, device=dev)
    rep = t.zeros((n, 8), dtype=t.int32, device=dev)
    fail = t.zeros(1, dtype=t.int32, device=dev)
    nr_apply = b.nr.clone()
    forms = {
        "compact": lambda: al.compact_runs(b.n, b.desc, b.slices, b.nr, b.off, b.dense),
        "clip": lambda: al.clip_device(n, b.dense, b.off, 1, b.nr, b.st, rec),
        "clip_apply": lambda: al.clip_device(n, b.slices, None, 6, nr_apply, b.st, rec_apply, apply=True, pairs=b.desc),
        "report": lambda: al.report_device(n, b.seq, b.desc, b.dense, b.off, 1, b.nr, b.ed, b.st, rep, fail, **skw),
    }
    samples = {k: [] for k in ["align"] + list(forms)}
    for it in range(launches + 1):                 # (the first round warms up)
        al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
        t.cuda.synchronize()
        ms = {"align": al.last_kernel_ms()}
        for k, fn in forms.items():
            if k == "clip_apply":
                nr_apply.copy_(b.nr)
                t.cuda.synchronize()
            ms[k] = timed(t, fn)
            if k == "clip_apply":                  # (the descriptors as they were: the next round aligns into the same slices)
                b.desc.copy_(desc0)
                t.cuda.synchronize()
        if it:
            for k, v in ms.items():
                samples[k].append(v)
    records = rec.cpu().numpy()
    assert (records == rec_apply.cpu().numpy()).all(), "apply mode's records differ"
    assert int(fail) == 0
    kept_runs = int(records[:, 5].astype(np.int64).sum())
    read_bytes = {"runs": 2 * runs, "counts_offsets_status": (4 + 8 + 4) * n}
    total = sum(read_bytes.values()) + 32 * n
    out = {"pairs": n, "read_len": L, "launches": launches, "runs": runs, "kept_runs": kept_runs, "pairs_clipped": int((records[:, 5] != b.nr.cpu().numpy()).sum()),
           "bytes_read": read_bytes, "bytes_written": 32 * n, "bytes_total": total}
    for k, v in samples.items():
        out[k + "_ms_median"] = med(v)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
    out["clip_bytes_per_s"] = total / (out["clip_ms_median"] / 1e3)
    out["clip_fraction_of_hbm_peak"] = out["clip_bytes_per_s"] / HBM_PEAK
    out["clip_over_report"] = out["clip_ms_median"] / out["report_ms_median"]
    out["clip_apply_over_report"] = out["clip_apply_ms_median"] / out["report_ms_median"]
    out["clip_apply_over_align"] = out["clip_apply_ms_median"] / out["align_ms_median"]
    log("%d x %d: align %.3f ms, compact %.3f, clip %.3f (apply, on the slices: %.3f), report %.3f; %.1f MB -> %.2f TB/s = %.1f %% of the HBM peak" % (
        n, L, out["align_ms_median"], out["compact_ms_median"], out["clip_ms_median"], out["clip_apply_ms_median"], out["report_ms_median"], total / 1e6,
        out["clip_bytes_per_s"] / 1e12, 100 * out["clip_fraction_of_hbm_peak"]))
    return out


def host_part(als, n, L, passes, seed):
    rows, tl, tw, rw = make_rows(n, L, seed)
    forms = [f for f in [("parent_off", "parent", False), ("this_off", "this", False), ("this_clip", "this", True)] if f[1] in als]

    def call(who, on):
        al = als[who]
        if on:
            al.set_clip()
        try:
            al.align_pairs_rows(rows, 0, tl, tw * 32, L)
            if on:
                assert (al.take_clip()["n_runs"] > 0).all()
        finally:
            if on:
                al.set_clip(None, False)
        return al.last_timing["total_ns"] / 1e6

    for _, who, on in forms:
        call(who, on)
    samples = {f: [] for f, _, _ in forms}
    for _ in range(passes):
        for f, who, on in forms:
            samples[f].append(call(who, on))
    out = {f: summary(v) for f, v in samples.items()}
    out.update(pairs=n, read_len=L, passes=passes)
    out["this_clip_over_this_off"] = out["this_clip"]["total_ms_median"] / out["this_off"]["total_ms_median"]
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
    ap.add_argument("--part", default="all", choices=["kernels", "host", "all"])
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
        out["align_pairs_100k_x_10kb" + ("_base_first" if args.base_first else "")] = host_part(als, n, 10000, args.launches, 3)
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
