"""CIGAR forms (scrg_ctx_set_cigar_form: the CIGAR text merged, or merged with = and X as M, rendered on the GPU): what they cost,
on one GPU, in one process.

    calls    scrg_align_pairs on 100 000 x 10 kb ONT-error pairs with the windowed, the merged and the M form on this library and
             (windowed) on --base-lib, a library built from the parent commit (scripts/ab.sh build); the calls ALTERNATE form by
             form, the median of --passes (9); per form the milliseconds per call and the bytes brought down (the wire's 12 per
             pair, the runs, the text).  The one condition: this library's windowed call lies within the +-4 % box-to-box spread
             of the parent's — ratio and the parent's own spread are recorded.  Two handles of one process do not get equal
             treatment, so the comparison is taken three ways: this library's handle made first, the
             parent's first (--base-first: 'align_pairs_100k_x_10kb_base_first'), and --only this / --only parent: ONE library
             per process, the processes alternating on the box ('solo_this_<k>' / 'solo_parent_<k>' with --tag k) — with
             --windowed-only the windowed call alone in the loop ('guard_this_<k>' / 'guard_parent_<k>'): calls of the other
             forms return texts of other sizes and leave the result-array pool in another state before every windowed call.
    kernels  the same text from the slices one scrg_align_device launch left, by scrg_cigar_text_lengths / scrg_cigar_text_render
             (the device pipelines' kernels: the walk of text_len_kernel / render_text_kernel in the two new forms, plus the checks
             of the render pass), timed with events on the handle's stream.
    trace    the batch through scrg_align_pairs, three calls per form: to be run under `rocprofv3 --kernel-trace --stats`, whose
             kernel_stats.csv has text_len_kernel<form> and render_text_kernel<form> side by side.

    python3 tests/tools/bench_cigar_form.py --base-lib ab_libs/lib_parent.so [--part calls|kernels|trace|all] [--base-first]
                                            [--only this|parent --tag K] [--scale 1.0] [--passes 9] [--out profiles/cigar_form.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.tools.bench_distance import DeviceBatch, log, make_aligner, make_rows, med

FORMS = ["windowed", "merged", "m"]
CALLS = [("parent_windowed", "parent", None)] + [("this_" + f, "this", f) for f in FORMS]


def summary(ms):
    return {"total_ms_median": med(ms), "total_ms_all": [round(x, 3) for x in ms], "range_ms": [min(ms), max(ms)],
            "spread": (max(ms) - min(ms)) / med(ms)}


def calls_part(als, n, L, passes, seed, windowed_only=False):
    rows, tl, tw, rw = make_rows(n, L, seed)
    calls = [c for c in CALLS if c[1] in als and (not windowed_only or c[0].endswith("windowed"))]

    def call(who, form):
        al = als[who]
        # (the parent's library has no such entry point: its call carries no keyword; this library's windowed call sets the form)
        arr = al.align_pairs_rows(rows, 0, tl, tw * 32, L, **({"cigar_form": form} if form else {}))
        text, runs = int(arr["cigar_offset"][n]), 2 * int(arr["run_offset"][n])
        return al.last_timing["total_ns"] / 1e6, {"cigar_text_bytes": text, "run_bytes": runs, "bytes_down": 12 * n + runs + text}

    for _, who, form in calls:                     # warm-up: buffers, result arrays
        call(who, form)
    samples, extra = {f: [] for f, _, _ in calls}, {}
    for _ in range(passes):
        for f, who, form in calls:
            ms, extra[f] = call(who, form)
            samples[f].append(ms)
    out = {f: dict(summary(samples[f]), **extra[f]) for f, _, _ in calls}
    out.update(pairs=n, read_len=L, passes=passes)
    if len(als) == 1:                              # (one library per process: the comparison is made from two such records)
        log("pairs %d x %d, %s alone: %s" % (n, L, list(als)[0], ", ".join("%s %.2f ms" % (f, out[f]["total_ms_median"]) for f, _, _ in calls)))
        return out
    p, t = out["parent_windowed"], out["this_windowed"]
    out["this_windowed_over_parent"] = t["total_ms_median"] / p["total_ms_median"]
    out["parent_spread"] = p["spread"]
    out["this_windowed_within_4_percent"] = bool(abs(out["this_windowed_over_parent"] - 1.0) <= 0.04)
    for f in FORMS[1:]:
        out["this_%s_over_this_windowed" % f] = out["this_" + f]["total_ms_median"] / t["total_ms_median"]
    log("pairs %d x %d: parent %.2f ms (spread %.3f), this windowed %.2f (x%.3f), merged %.2f, m %.2f; text %.1f / %.1f / %.1f MB" % (
        n, L, p["total_ms_median"], p["spread"], t["total_ms_median"], out["this_windowed_over_parent"], out["this_merged"]["total_ms_median"],
        out["this_m"]["total_ms_median"], t["cigar_text_bytes"] / 1e6, out["this_merged"]["cigar_text_bytes"] / 1e6, out["this_m"]["cigar_text_bytes"] / 1e6))
    return out


def kernels_part(al, n, L, launches, seed):
    """The device pipelines' two kernels alone, from the slices of one scrg_align_device launch (stride 6)."""
    b = DeviceBatch(al, n, L, seed)
    t = b.torch
    al.set_stream(0)
    b.arena()
    al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, W=64, O=33, text_stride_words=64, read_stride_words=64)
    t.cuda.synchronize()
    runs = int(b.nr.sum())
    out = {"pairs": n, "read_len": L, "launches": launches, "runs": runs, "run_bytes_read_per_pass": 2 * runs}
    tlen = t.zeros(n, dtype=t.int64, device=b.ed.device)
    bad = t.zeros(1, dtype=t.int32, device=b.ed.device)
    for form in FORMS:
        al.cigar_text_lengths(form, n, b.slices, None, 6, b.nr, tlen, pairs=b.desc)
        off = t.cumsum(tlen, 0) - tlen
        total = int(tlen.sum())
        text = t.empty(total, dtype=t.uint8, device=b.ed.device)
        t_len, t_render = [], []
        for _ in range(launches + 1):
            e = [t.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            al.cigar_text_lengths(form, n, b.slices, None, 6, b.nr, tlen, pairs=b.desc)
            e[1].record()
            al.cigar_text_render(form, n, b.slices, None, 6, b.nr, tlen, off, text, bad, pairs=b.desc)
            e[2].record()
            t.cuda.synchronize()
            t_len.append(e[0].elapsed_time(e[1]))
            t_render.append(e[1].elapsed_time(e[2]))
        assert int(bad) == 0
        out[form] = {"cigar_len_ms_median": med(t_len[1:]), "cigar_render_ms_median": med(t_render[1:]), "text_bytes_written": total,
                     "render_ms_all": [round(x, 4) for x in t_render[1:]]}
        log("%s: cigar_len %.3f ms, cigar_render %.3f ms, %.1f MB of text from %.1f MB of runs" % (
            form, out[form]["cigar_len_ms_median"], out[form]["cigar_render_ms_median"], total / 1e6, 2 * runs / 1e6))
    return out


def trace_part(al, n, L, seed):
    rows, tl, tw, rw = make_rows(n, L, seed)
    for form in FORMS:
        for _ in range(3):
            al.align_pairs_rows(rows, 0, tl, tw * 32, L, cigar_form=form)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--part", default="all", choices=["calls", "kernels", "trace", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--base-first", action="store_true", help="make the handle of --base-lib first (results under '<key>_base_first')")
    ap.add_argument("--only", default=None, choices=["this", "parent"], help="--part calls with ONE library in the process")
    ap.add_argument("--tag", default="1", help="--only: the record's suffix")
    ap.add_argument("--windowed-only", action="store_true", help="--only: the windowed call alone in the loop (records 'guard_*')")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n10k = int(100_000 * args.scale)
    assert args.base_lib or not (args.base_first or args.only == "parent"), "--base-lib: a library built from the parent commit"
    parent = make_aligner(args.base_lib) if args.base_first or args.only == "parent" else None
    this = make_aligner(None) if args.only != "parent" else None
    if args.part == "trace":
        trace_part(this, n10k, 10_000, 1)
        return
    doc = {}

    def save():                                    # (after every part: a later part's failure does not lose an earlier one's figures)
        if not args.out:
            return
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(doc)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")

    if args.part in ("calls", "all"):
        if args.only:
            key = "%s_%s_%s" % ("guard" if args.windowed_only else "solo", args.only, args.tag)
            doc[key] = calls_part({args.only: this or parent}, n10k, 10_000, args.passes, 1, args.windowed_only)
        else:
            assert args.base_lib, "--base-lib: a library built from the parent commit"
            als = {"parent": parent or make_aligner(args.base_lib), "this": this}
            doc["align_pairs_100k_x_10kb" + ("_base_first" if args.base_first else "")] = calls_part(als, n10k, 10_000, args.passes, 1)
        save()
    if args.part in ("kernels", "all"):
        doc["kernels_100k_x_10kb"] = kernels_part(this, n10k, 10_000, 9, 1)
        save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
