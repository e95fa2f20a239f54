"""Difference strings (scrg_ctx_set_diff: MD / cs rendered on the GPU next to the CIGAR text): what they cost, on one GPU, in
one process.

    calls    scrg_align_pairs on 100 000 x 10 kb ONT-error pairs and align_mapping on 1 M x 150 bp x 4 candidates, each with the
             kind off, with md and with cs on this library and (kind off) on --base-lib, a library built from the parent commit
             (scripts/ab.sh build); the calls ALTERNATE form by form, the median of --passes (9).  The one condition: this
             library with the kind off lies within the spread of the parent's own calls — ratio and spread are recorded.
    guard    the same two calls with the off forms alone (parent off, this off): the md and cs calls of `calls` run on this
             library only and change the state of its result-array pool and buffers before every off call.
    kernels  diff_len_kernel + diff_render_kernel alone on the 100 000 x 10 kb batch (the slices scrg_align_device left), timed with
             events on the handle's stream, and the bytes they read and write.  text_len_kernel / render_text_kernel have no entry
             point of their own: --part trace is the same batch through scrg_align_pairs, to be run under
             `rocprofv3 --kernel-trace --stats`, whose kernel_stats.csv has all four kernels' times side by side.
    host     scrg_diff_from_runs over the same 100 000 pairs on 16 host threads: what a caller pays without the feature.

    python3 tests/tools/bench_diff.py --base-lib ab_libs/lib_parent.so [--base-first] [--part calls|kernels|host|trace|all]
                                      [--scale 1.0] [--passes 9] [--out profiles/diff_strings.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

from scrooge_amd import api
from tests.tools.bench_best import workload_a
from tests.tools.bench_distance import DeviceBatch, log, make_aligner, make_rows, med


def summary(ms):
    return {"total_ms_median": med(ms), "total_ms_all": [round(x, 3) for x in ms], "range_ms": [min(ms), max(ms)],
            "spread": (max(ms) - min(ms)) / med(ms)}


def guard(out):
    """this library with the kind off against the parent: the ratio of the medians, and whether it lies within the parent's spread"""
    p, t = out["parent_off"], out["this_off"]
    out["this_off_over_parent_off"] = t["total_ms_median"] / p["total_ms_median"]
    out["parent_spread"] = p["spread"]
    out["this_off_within_parent_range"] = bool(p["range_ms"][0] <= t["total_ms_median"] <= p["range_ms"][1])
    for k in ("md", "cs"):
        if "this_" + k not in out:
            continue
        out["this_%s_over_this_off" % k] = out["this_" + k]["total_ms_median"] / t["total_ms_median"]


ALL_FORMS = [("parent_off", "parent", None), ("this_off", "this", None), ("this_md", "this", "md"), ("this_cs", "this", "cs")]
# the guard alone: off against off and nothing else in the loop — the md and cs calls of ALL_FORMS run on this library only and
# leave its pool of result arrays and its slots' buffers in another state than the parent's before every off call
OFF_FORMS = ALL_FORMS[:2]
FORMS = ALL_FORMS


def run_forms(call, passes):
    for f, who, kind in FORMS:                     # warm-up: buffers, result arrays
        call(who, kind)
    samples = {f: [] for f, _, _ in FORMS}
    extra = {}
    for _ in range(passes):
        for f, who, kind in FORMS:
            ms, info = call(who, kind)
            samples[f].append(ms)
            extra[f] = info
    out = {f: dict(summary(samples[f]), **extra[f]) for f, _, _ in FORMS}
    guard(out)
    return out


def pairs_part(als, n, L, passes, seed):
    rows, tl, tw, rw = make_rows(n, L, seed)

    def call(who, kind):
        al = als[who]
        arr = al.align_pairs_rows(rows, 0, tl, tw * 32, L, **({"diff": kind} if kind else {}))
        info = {"cigar_text_bytes": int(arr["cigar_offset"][n]), "run_bytes": 2 * int(arr["run_offset"][n])}
        if kind:
            info["diff_text_bytes"] = len(arr["diff_text"])
        return al.last_timing["total_ns"] / 1e6, info

    out = dict(run_forms(call, passes), pairs=n, read_len=L, passes=passes)
    log("pairs %d x %d: parent %.2f ms (spread %.3f), this off %.2f (x%.3f, within the parent's range: %s)%s" % (
        n, L, out["parent_off"]["total_ms_median"], out["parent_spread"], out["this_off"]["total_ms_median"], out["this_off_over_parent_off"],
        out["this_off_within_parent_range"], "".join(", %s %.2f" % (k, out["this_" + k]["total_ms_median"]) for k in ("md", "cs") if "this_" + k in out)))
    return out


def mapping_part(als, n_reads, passes):
    genome, reads, cands = workload_a(n_reads)
    nr, L = reads.shape
    co = np.arange(nr + 1, dtype=np.uint64) * np.uint64(cands.shape[1])
    cs = cands.reshape(-1).astype(np.uint64)
    n = int(co[nr])
    for al in als.values():
        al.set_genome_array(genome)

    def call(who, kind):
        al = als[who]
        arr = al.align_mapping_rows(None, reads, L, co, cs, **({"diff": kind} if kind else {}))
        info = {"cigar_text_bytes": int(arr["cigar_offset"][n])}
        if kind:
            info["diff_text_bytes"] = len(arr["diff_text"])
        return al.last_timing["total_ns"] / 1e6, info

    out = dict(run_forms(call, passes), reads=nr, read_len=L, pairs=n, passes=passes)
    log("mapping %d pairs: parent %.2f ms (spread %.3f), this off %.2f (x%.3f, within the parent's range: %s)%s" % (
        n, out["parent_off"]["total_ms_median"], out["parent_spread"], out["this_off"]["total_ms_median"], out["this_off_over_parent_off"],
        out["this_off_within_parent_range"], "".join(", %s %.2f" % (k, out["this_" + k]["total_ms_median"]) for k in ("md", "cs") if "this_" + k in out)))
    return out


def kernels_part(al, n, L, launches, seed):
    """The two kernels alone, from the slices of one scrg_align_device launch (lane-interleaved sequences, stride 6)."""
    b = DeviceBatch(al, n, L, seed)
    t = b.torch
    al.set_stream(0)
    b.arena()
    kw = dict(W=64, O=33, text_stride_words=64, read_stride_words=64)
    al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
    t.cuda.synchronize()
    runs = int(b.nr.sum())
    out = {"pairs": n, "read_len": L, "launches": launches, "runs": runs, "run_bytes_read_per_pass": 2 * runs}
    dlen = t.zeros(n, dtype=t.int64, device=b.ed.device)
    bad = t.zeros(1, dtype=t.int32, device=b.ed.device)
    skw = dict(text_stride_words=64, read_stride_words=64)
    for kind in ("md", "cs"):
        al.diff_lengths(kind, n, b.seq, b.desc, b.slices, None, 6, b.nr, dlen, **skw)
        off = t.cumsum(dlen, 0) - dlen
        total = int(dlen.sum())
        text = t.empty(total, dtype=t.uint8, device=b.ed.device)
        t_len, t_render = [], []
        for _ in range(launches + 1):
            e = [t.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            al.diff_lengths(kind, n, b.seq, b.desc, b.slices, None, 6, b.nr, dlen, **skw)
            e[1].record()
            al.diff_render(kind, n, b.seq, b.desc, b.slices, None, 6, b.nr, dlen, off, text, bad, **skw)
            e[2].record()
            t.cuda.synchronize()
            t_len.append(e[0].elapsed_time(e[1]))
            t_render.append(e[1].elapsed_time(e[2]))
        assert int(bad) == 0
        out[kind] = {"diff_len_ms_median": med(t_len[1:]), "diff_render_ms_median": med(t_render[1:]), "text_bytes_written": total,
                     "length_bytes_written": 8 * n, "render_ms_all": [round(x, 4) for x in t_render[1:]]}
        log("%s: diff_len %.3f ms, diff_render %.3f ms, %.1f MB of strings from %.1f MB of runs" % (
            kind, out[kind]["diff_len_ms_median"], out[kind]["diff_render_ms_median"], total / 1e6, 2 * runs / 1e6))
    return out


HOST_LOOP_SRC = r"""
#include <atomic>
#include <thread>
#include <vector>
#include "scrooge_amd_io.h"
// scrg_diff_from_runs over n pairs, dealt to `threads` threads: pair p = (rows + p * stride, text_len[p]) and the read L bytes at
// read_off of the same row, its runs runs[run_off[p] .. run_off[p + 1]).  -> the bytes of all strings, or -1 if a call failed
extern "C" long long diff_loop(int kind, unsigned long long n, const char* rows, unsigned long long stride, const long long* text_len,
                               unsigned long long read_off, unsigned long long L, const scrg_run* runs, const long long* run_off, int threads)
{
    std::atomic<long long> total{0};
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    for (int w = 0; w < threads; w++)
        th.emplace_back([&, w] {
            std::vector<char> buf(8 * L + 64);
            long long made = 0;
            for (unsigned long long p = w; p < n; p += threads) {
                uint64_t len = 0;
                if (scrg_diff_from_runs(kind, rows + p * stride, (uint64_t)text_len[p], rows + p * stride + read_off, L, runs + run_off[p],
                                        (uint64_t)(run_off[p + 1] - run_off[p]), buf.data(), buf.size(), &len) != SCRG_OK)
                    failed.store(1);
                made += (long long)len;
            }
            total += made;
        });
    for (auto& t : th) t.join();
    return failed.load() ? -1 : total.load();
}
"""


def build_host_loop():
    """The loop above as a small shared library next to the in-tree one (g++, as the shim tests build theirs)."""
    import subprocess
    import tempfile
    d = tempfile.mkdtemp(prefix="scrg_diff_loop_")
    src, so = os.path.join(d, "loop.cpp"), os.path.join(d, "libdiffloop.so")
    open(src, "w").write(HOST_LOOP_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir,
                           "-lscrooge_amd", "-Wl,-rpath," + libdir, "-o", so])
    fn = C.CDLL(so).diff_loop
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_int, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_int]
    return fn


def host_part(al, n, L, seed, threads=16):
    """scrg_diff_from_runs over the pairs of one scrg_align_pairs call, the pairs dealt to `threads` C++ threads: what a caller
    pays on the host without the feature."""
    rows, tl, tw, rw = make_rows(n, L, seed)
    arr = al.align_pairs_rows(rows, 0, tl, tw * 32, L, outputs=api.SCRG_OUT_RUNS)
    ro, runs = np.ascontiguousarray(arr["run_offset"].astype(np.int64)), np.ascontiguousarray(arr["runs"])
    tl64 = np.ascontiguousarray(tl, dtype=np.int64)
    loop = build_host_loop()
    out = {"pairs": n, "read_len": L, "threads": threads, "driver": "C++ threads"}
    for kind in ("md", "cs"):
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            total = loop(api._diff_kind(kind), n, rows.ctypes.data, rows.shape[1], tl64.ctypes.data, tw * 32, L, runs.ctypes.data, ro.ctypes.data, threads)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert total > 0
        out[kind] = {"ms": med(ms), "ms_all": [round(x, 2) for x in ms], "text_bytes": int(total)}
        log("host %s: %.1f ms on %d threads, %.1f MB" % (kind, out[kind]["ms"], threads, total / 1e6))
    return out


def trace_part(al, n, L, seed):
    """The batch through scrg_align_pairs with md, then cs, three calls each: for a run under the profiler's kernel trace."""
    rows, tl, tw, rw = make_rows(n, L, seed)
    for kind in ("md", "cs"):
        for _ in range(3):
            al.align_pairs_rows(rows, 0, tl, tw * 32, L, diff=kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--part", default="all", choices=["calls", "guard", "pairs", "mapping", "kernels", "host", "trace", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--base-first", action="store_true", help="make the handle of --base-lib first: the two handles of one process do not get "
                    "the same hardware queues, so the guard is taken in both orders (the results go under '<key>_base_first')")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n10k, n_reads = int(100_000 * args.scale), int(1_000_000 * args.scale)
    parent = make_aligner(args.base_lib) if args.base_lib and args.base_first else None
    this = make_aligner(None)
    global FORMS
    sfx = "_base_first" if args.base_first else ""
    if args.part == "guard":                       # both calls, the off forms only: results under 'off_only_<key>'
        FORMS, args.part, sfx = OFF_FORMS, "calls", sfx
        pre = "off_only_"
    else:
        pre = ""
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

    if args.part in ("calls", "pairs", "mapping", "all"):
        assert args.base_lib, "--base-lib: a library built from the parent commit"
        als = {"parent": parent or make_aligner(args.base_lib), "this": this}
        if args.part != "mapping":
            doc[pre + "align_pairs_100k_x_10kb" + sfx] = pairs_part(als, n10k, 10_000, args.passes, 1)
            save()
        if args.part != "pairs":
            doc[pre + "align_mapping_1M_x_150bp_x_4" + sfx] = mapping_part(als, n_reads, args.passes)
            save()
        for al in als.values():
            al.clear_genome()
    if args.part in ("kernels", "all"):
        doc["kernels_100k_x_10kb"] = kernels_part(this, n10k, 10_000, 9, 1)
        save()
    if args.part in ("host", "all"):
        doc["diff_from_runs_100k_x_10kb"] = host_part(this, n10k, 10_000, 1)
    print(json.dumps(doc))
    save()


if __name__ == "__main__":
    main()
