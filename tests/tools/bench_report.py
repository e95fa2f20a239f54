"""The alignment report pass (scrg_report_device, report_kernels.hip) timed on one GPU, in one process.

kernels  single launches on device buffers (lane-interleaved sequences, dense runs), medians of --launches (9) launches, the forms
         ALTERNATING launch by launch so that they share the box's state:
             align        scrg_align_device (its own events: scrg_last_kernel_ms)
             compact      scrg_compact_runs
             report       scrg_report_device on the dense runs — the word-parallel base check
             report_pb    the same kernel's one-base-at-a-time build (the test build, scrg_params.reserved[0] = 16384): the A/B that
                          justifies the word-parallel form, or retires it
             md_len       scrg_diff_lengths (md) on the same dense runs: it reads the same runs and no '=' base
         for 100 000 x 10 kb ONT-error pairs at 64/33 and for 4 M x 150 bp; with the bytes the pass must read (runs, the bases of
         both sequences its runs name, descriptors, counts, offsets, edit distances) and writes (32 per pair), and that traffic over
         the measured time as a fraction of the HBM roof (8 TB/s peak; ~6.3 TB/s is what a copy reaches).
host     scrg_align_pairs on 100 000 x 10 kb pairs with the setting on and off on this library, and off on --base-lib, a library built
         from the parent commit, alternating call by call: the off path is held against the parent's (ratio of the medians, and
         whether it lies within the +-4 % box-to-box spread the README states).  Two handles of one process do not get equal
         treatment (tests/tools/bench_diff.py): --base-first makes the parent's handle first; the profile holds both orders.
guard    the same with the two off forms alone in the loop (keys off_only_*): no call with the setting on runs between them.

    python3 tests/tools/bench_report.py [--base-lib ab_libs/lib_parent.so] [--base-first] [--part kernels|host|guard|all] [--scale 1.0] [--launches 9]
                                        [--out profiles/pair_report.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

import scrooge_amd
from tests.tools.bench_distance import DeviceBatch, log, make_aligner, make_rows, med

HBM_PEAK = 8.0e12


def timed(t, fn):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    t.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernels_part(al, al_select, n, L, launches, seed):
    b = DeviceBatch(al, n, L, seed)
    t = b.torch
    dev = b.ed.device
    al.set_stream(0)
    al_select.set_stream(0)
    b.arena()
    kw = dict(W=64, O=33, text_stride_words=64, read_stride_words=64)
    skw = dict(text_stride_words=64, read_stride_words=64)
    al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
    t.cuda.synchronize()
    assert int(b.st.max()) == 0
    b.off[1:] = t.cumsum(b.nr.to(t.int64), 0)
    runs = int(b.off[-1])
    assert 2 * runs <= b.dense.numel()
    rep = t.zeros((n, 8), dtype=t.int32, device=dev)
    rep_pb = t.zeros((n, 8), dtype=t.int32, device=dev)
    fail = t.zeros(1, dtype=t.int32, device=dev)
    dlen = t.zeros(n, dtype=t.int64, device=dev)
    forms = {
        "compact": lambda: al.compact_runs(b.n, b.desc, b.slices, b.nr, b.off, b.dense),
        "report": lambda: al.report_device(n, b.seq, b.desc, b.dense, b.off, 1, b.nr, b.ed, b.st, rep, fail, **skw),
        "report_pb": lambda: al_select.report_device(n, b.seq, b.desc, b.dense, b.off, 1, b.nr, b.ed, b.st, rep_pb, fail, per_base=True, **skw),
        "md_len": lambda: al.diff_lengths("md", n, b.seq, b.desc, b.dense, b.off, 1, b.nr, dlen, **skw),
    }
    samples = {k: [] for k in ["align"] + list(forms)}
    for it in range(launches + 1):                 # (the first round warms up)
        al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
        t.cuda.synchronize()
        ms = {"align": al.last_kernel_ms()}
        for k, fn in forms.items():
            ms[k] = timed(t, fn)
        if it:
            for k, v in ms.items():
                samples[k].append(v)
    records = rep.cpu().numpy().view(np.uint32)
    assert int(fail) == 0 and (records[:, 6] == 0).all(), "a pair failed its check"
    assert (rep_pb.cpu().numpy().view(np.uint32) == records).all(), "the per-base build differs"
    cons_t = int(records[:, 0].astype(np.int64).sum() + records[:, 1].astype(np.int64).sum() + records[:, 3].astype(np.int64).sum())
    cons_q = int(records[:, 0].astype(np.int64).sum() + records[:, 1].astype(np.int64).sum() + records[:, 2].astype(np.int64).sum())
    read_bytes = {"runs": 2 * runs, "sequences": (cons_t + cons_q) // 4, "descriptors": 48 * n, "counts_offsets_distances_status": (4 + 8 + 8 + 4) * n}
    total = sum(read_bytes.values()) + 32 * n
    out = {"pairs": n, "read_len": L, "launches": launches, "runs": runs, "bytes_read": read_bytes, "bytes_written": 32 * n, "bytes_total": total}
    for k, v in samples.items():
        out[k + "_ms_median"] = med(v)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
    out["report_bytes_per_s"] = total / (out["report_ms_median"] / 1e3)
    out["report_fraction_of_hbm_peak"] = out["report_bytes_per_s"] / HBM_PEAK
    out["report_over_md_len"] = out["report_ms_median"] / out["md_len_ms_median"]
    out["report_pb_over_report"] = out["report_pb_ms_median"] / out["report_ms_median"]
    out["report_over_align"] = out["report_ms_median"] / out["align_ms_median"]
    log("%d x %d: align %.3f ms, compact %.3f, report %.3f (per base %.3f, x%.2f), md_len %.3f; %.1f MB -> %.2f TB/s = %.1f %% of the HBM peak" % (
        n, L, out["align_ms_median"], out["compact_ms_median"], out["report_ms_median"], out["report_pb_ms_median"], out["report_pb_over_report"],
        out["md_len_ms_median"], total / 1e6, out["report_bytes_per_s"] / 1e12, 100 * out["report_fraction_of_hbm_peak"]))
    return out


def summary(ms):
    return {"total_ms_median": med(ms), "total_ms_all": [round(x, 3) for x in ms], "range_ms": [min(ms), max(ms)]}


def host_part(als, n, L, passes, seed, off_only=False):
    rows, tl, tw, rw = make_rows(n, L, seed)
    forms = [("parent_off", "parent", False), ("this_off", "this", False), ("this_report", "this", True)]
    forms = [f for f in forms if f[1] in als and not (off_only and f[2])]

    def call(who, on):
        al = als[who]
        arr = al.align_pairs_rows(rows, 0, tl, tw * 32, L, **({"report": True} if on else {}))
        if on:
            assert (arr["report"]["verdict"] == 0).all()
        return al.last_timing["total_ns"] / 1e6

    for _, who, on in forms:
        call(who, on)
    samples = {f: [] for f, _, _ in forms}
    for _ in range(passes):
        for f, who, on in forms:
            samples[f].append(call(who, on))
    out = {f: summary(v) for f, v in samples.items()}
    out.update(pairs=n, read_len=L, passes=passes)
    if "this_report" in out:
        out["this_report_over_this_off"] = out["this_report"]["total_ms_median"] / out["this_off"]["total_ms_median"]
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
    if args.part in ("kernels", "all"):
        scrooge_amd.build_library(variant="select")
        sel = scrooge_amd.Aligner(0, variant="select")
        out["kernels_100k_x_10kb"] = kernels_part(this, sel, max(64, int(100000 * args.scale)), 10000, args.launches, 1)
        out["kernels_4M_x_150bp"] = kernels_part(this, sel, max(64, int(4000000 * args.scale)), 150, args.launches, 2)
        sel.close()
    als = {"this": this}
    if parent is not None:
        als["parent"] = parent
    if args.part == "guard":
        out["off_only_align_pairs_100k_x_10kb" + ("_base_first" if args.base_first else "")] = host_part(als, max(64, int(100000 * args.scale)), 10000,
                                                                                                         args.launches, 3, off_only=True)
    if args.part in ("host", "all"):
        out["align_pairs_100k_x_10kb" + ("_base_first" if args.base_first else "")] = host_part(als, max(64, int(100000 * args.scale)), 10000, args.launches, 3)
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
