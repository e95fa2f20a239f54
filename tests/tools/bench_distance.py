"""Distance-only mode (SCRG_OUT_DISTANCE) against the parent commit's runs mode, on one GPU, in one process.

Kernel: single launches on device buffers (lane-interleaved layout, one stream), the median of --launches (>= 7), the forms
ALTERNATING launch by launch so that they share the box's state:
    dist          scrg_align_device_distance of this library
    this_runs     scrg_align_device (+ scrg_compact_runs, timed on its own) of this library
    parent_runs   the same of --base-lib, a library built from the parent commit (scripts/ab.sh build, SCRG_LIB)
for 100 000 x 10 kb ONT-error pairs at W/O = 64/33 (the condition: dist <= 0.90 x parent_runs' align launch, and this_runs within
the box's spread of parent_runs), at 256/129, and for 4 M x 150 bp at 64/33 (both recorded without a threshold).
Host: scrg_align_pairs on 100 000 x 10 kb pairs, pairs per second and bytes brought down per call, with the flag (this library)
next to the parent's SCRG_OUT_RUNS.
--stats-lib: a -DSCRG_STATS build of this library: the kernels' phase counters (cycles per round in fetch / set-up / table /
traceback) of one runs launch and one distance launch at 64/33, for saying where a difference went.

    python3 tests/tools/bench_distance.py --base-lib ab_libs/lib_parent.so [--stats-lib ab_libs/lib_stats.so] [--part kernel|small|host|stats|all]
                                          [--scale 1.0] [--launches 7] [--out profiles/distance_only.json]"""
import argparse
import ctypes as C
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


def make_aligner(path):
    """A handle of another build of the library next to the in-tree one (it keeps the library it was made with).  A build of the
    parent commit speaks an older interface version: only entry points that did not change are called on it, by hand."""
    import torch  # noqa: F401  (before any build of the library is loaded: api.load_library says why)
    if path is None:
        return scrooge_amd.Aligner(0)
    saved, saved_v, api._LIB = api._LIB, api.SCRG_ABI_VERSION, None
    os.environ["SCRG_LIB"] = path
    try:
        api.SCRG_ABI_VERSION = C.CDLL(path).scrg_abi_version()
        return scrooge_amd.Aligner(0)
    finally:
        del os.environ["SCRG_LIB"]
        api._LIB, api.SCRG_ABI_VERSION = saved, saved_v


def make_rows(n, L, seed):
    """n ONT-error pairs of read length L as one uint8 array (row p: text | read), lengths."""
    rng = np.random.Generator(np.random.PCG64(seed))
    err, ratio = synth.PROFILES["ont"]
    base_n = min(n, 2048)                      # distinct pairs; the batch repeats them in a seeded order (the kernels cannot tell)
    pairs = [synth.make_pair(L, err, ratio, rng) for _ in range(base_n)]
    tw, rw = (max(len(t) for t, _ in pairs) + 31) // 32, (L + 31) // 32
    rows = np.zeros((base_n, (tw + rw) * 32), dtype=np.uint8)
    tl = np.zeros(base_n, dtype=np.int64)
    for k, (t, q) in enumerate(pairs):
        rows[k, :len(t)] = synth.BASES[t]
        rows[k, tw * 32: tw * 32 + len(q)] = synth.BASES[q]
        tl[k] = len(t)
    pick = rng.integers(0, base_n, n)
    return rows[pick], tl[pick], tw, rw


class DeviceBatch:
    def __init__(self, al, n, L, seed):
        import torch
        self.torch, self.n, self.L = torch, n, L
        dev = torch.device("cuda", 0)
        rows, tl, tw, rw = make_rows(n, L, seed)
        wpr = tw + rw
        al.set_stream(0)
        self.seq = torch.zeros(((n + 63) // 64) * 64 * wpr + api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        CH = 1 << 16                          # (whole groups of 64 rows at a time: the ASCII copy stays small)
        for a in range(0, n, CH):
            part = torch.from_numpy(rows[a: a + CH]).to(dev).view(-1)
            al.pack_planar_groups(part, min(CH, n - a), wpr, self.seq[(a // 64) * 64 * wpr:], bad)
        assert int(bad) == 0
        idx = np.arange(n, dtype=np.int64)
        self.cap = (2 * L + 16 + 15) // 16 * 16
        desc = np.stack([32 * (((idx // 64) * wpr) * 64 + idx % 64), tl, 32 * (((idx // 64) * wpr + tw) * 64 + idx % 64), np.full(n, L),
                         idx * self.cap, np.full(n, self.cap)], axis=1).astype(np.int64)
        self.desc = torch.from_numpy(desc).to(dev)
        self.ed = torch.empty(n, dtype=torch.int64, device=dev)
        self.st = torch.empty(n, dtype=torch.int32, device=dev)
        self.te = torch.empty(n, dtype=torch.int32, device=dev)
        self.nr = torch.empty(n, dtype=torch.int32, device=dev)
        self.slices = self.dense = self.off = None

    def arena(self):
        if self.slices is None:
            t = self.torch
            dev = self.ed.device
            self.slices = t.empty(self.n * self.cap * 2, dtype=t.uint8, device=dev)
            self.dense = t.empty(self.n * self.cap * 2 // 4, dtype=t.uint8, device=dev)      # (10 % error: ~0.65 L runs of 2 L + 16)
            self.off = t.zeros(self.n + 1, dtype=t.int64, device=dev)


def launch(al, b, form, W, O, waves=0):
    """-> (align ms, compaction ms)."""
    t = b.torch
    kw = dict(W=W, O=O, text_stride_words=64, read_stride_words=64)
    if waves:
        kw["waves_per_cu"] = waves
    if form.startswith("dist"):
        al.align_device_distance(b.n, b.seq, b.desc, b.ed, b.te, b.st, **kw)
        t.cuda.synchronize()
        return al.last_kernel_ms(), 0.0
    b.arena()
    al.align_device(b.n, b.seq, b.desc, b.slices, b.ed, b.nr, b.st, **kw)
    t.cuda.synchronize()
    ms = al.last_kernel_ms()
    b.off[1:] = t.cumsum(b.nr.to(t.int64), 0)
    assert int(b.off[-1]) * 2 <= b.dense.numel()
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    al.compact_runs(b.n, b.desc, b.slices, b.nr, b.off, b.dense)
    e1.record()
    t.cuda.synchronize()
    return ms, e0.elapsed_time(e1)


def med(x):
    return float(sorted(x)[len(x) // 2])


def kernel_part(als, n, L, W, O, launches, seed, extra_waves=0):
    b = DeviceBatch(als["this"], n, L, seed)
    for al in als.values():
        al.set_stream(0)                                    # (every handle on the stream the batch's tensors live on)
    forms = [("dist", "this"), ("parent_runs", "parent"), ("this_runs", "this")]
    if "extra" in als:                                      # (an experimental build of the distance kernel, e.g. another occupancy)
        forms.append(("dist_extra", "extra"))
    waves = {"dist_extra": extra_waves}
    ref = {}
    for f, who in forms:                                    # warm-up, and the forms agree on every distance
        launch(als[who], b, f, W, O, waves.get(f, 0))
        ref[f] = (b.ed.clone(), b.st.clone())
    assert all(bool((ref[f][0] == ref["parent_runs"][0]).all()) for f, _ in forms)
    assert bool((ref["dist"][0] == ref["parent_runs"][0]).all()) and bool((ref["this_runs"][0] == ref["parent_runs"][0]).all())
    assert not bool(ref["dist"][1].any())
    samples = {f: [] for f, _ in forms}
    for _ in range(launches):
        for f, who in forms:
            samples[f].append(launch(als[who], b, f, W, O, waves.get(f, 0)))
    out = {"pairs": n, "read_len": L, "W": W, "O": O, "launches": launches}
    for f, _ in forms:
        a = [s[0] for s in samples[f]]
        out[f] = {"align_ms_median": med(a), "align_ms_all": [round(x, 4) for x in a], "align_ms_spread": (max(a) - min(a)) / med(a)}
        if not f.startswith("dist"):
            out[f]["compact_ms_median"] = med([s[1] for s in samples[f]])
    p = out["parent_runs"]["align_ms_median"]
    out["dist_over_parent_align"] = out["dist"]["align_ms_median"] / p
    out["dist_over_parent_align_plus_compact"] = out["dist"]["align_ms_median"] / (p + out["parent_runs"]["compact_ms_median"])
    out["this_runs_over_parent_runs"] = out["this_runs"]["align_ms_median"] / p
    if "extra" in als:
        out["dist_extra_over_parent_align"] = out["dist_extra"]["align_ms_median"] / p
        out["dist_extra"]["waves_per_cu"] = extra_waves
    out["device_arena_bytes"] = {"runs": int(n) * b.cap * 2, "dist": 0}
    log("%d x %d bp at %d/%d: dist %.3f ms, parent runs %.3f (+ %.3f compaction), this runs %.3f  ->  dist / parent %.3f, this runs / parent runs %.3f"
        % (n, L, W, O, out["dist"]["align_ms_median"], p, out["parent_runs"]["compact_ms_median"], out["this_runs"]["align_ms_median"],
           out["dist_over_parent_align"], out["this_runs_over_parent_runs"]))
    return out


def host_call(al, rows, tl, tw, L, outputs):
    """scrg_align_pairs by hand (the result struct of an older build is read up to the fields it has) -> (total ms, kernel ms, bytes down)."""
    n, stride = rows.shape
    base = rows.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    tp, qp = base.astype(np.uint64), (base + np.uint64(tw * 32)).astype(np.uint64)
    tlen, qlen = np.ascontiguousarray(tl, dtype=np.uint64), np.full(n, L, dtype=np.uint64)
    pp, up = C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)
    p = al._params({"outputs": outputs})
    res = C.POINTER(api.Result)()
    st = al.lib.scrg_align_pairs(al.h, C.byref(p), n, C.cast(tp.ctypes.data, pp), C.cast(tlen.ctypes.data, up), C.cast(qp.ctypes.data, pp),
                                 C.cast(qlen.ctypes.data, up), C.byref(res))
    assert st == 0, st
    r = res.contents
    if outputs & api.SCRG_OUT_DISTANCE:
        down = 16 * n                                          # ed 8, status 4, text end 4 per pair
    else:
        down = 8 * n + 2 * int(r.run_offset[n])                # SCRG_OUT_RUNS: the wire (ed, run count) + the runs
    out = (r.total_ns / 1e6, r.kernel_ns / 1e6, down)
    al.lib.scrg_result_free(res)
    return out


def host_part(als, n, L, passes, seed):
    rows, tl, tw, rw = make_rows(n, L, seed)
    forms = [("dist", "this", api.SCRG_OUT_DISTANCE), ("parent_runs", "parent", api.SCRG_OUT_RUNS), ("this_runs", "this", api.SCRG_OUT_RUNS)]
    for f, who, o in forms:
        host_call(als[who], rows, tl, tw, L, o)
    samples = {f: [] for f, _, _ in forms}
    for _ in range(passes):
        for f, who, o in forms:
            samples[f].append(host_call(als[who], rows, tl, tw, L, o))
    out = {"pairs": n, "read_len": L, "passes": passes}
    for f, _, _ in forms:
        tot = med([s[0] for s in samples[f]])
        out[f] = {"total_ms_median": tot, "pairs_per_s": n / tot * 1e3, "kernel_ms_median": med([s[1] for s in samples[f]]), "d2h_bytes": samples[f][0][2]}
        log("host %-12s %.1f ms per call, %.2f M pairs/s, %.1f MB down" % (f, tot, out[f]["pairs_per_s"] / 1e6, out[f]["d2h_bytes"] / 1e6))
    out["dist_over_parent_runs_pairs_per_s"] = out["dist"]["pairs_per_s"] / out["parent_runs"]["pairs_per_s"]
    return out


def stats_part(path, n, L, seed):
    al = make_aligner(path)
    assert al.lib.scrg_build_flags() & 1, "--stats-lib must be a -DSCRG_STATS build"
    b = DeviceBatch(al, n, L, seed)
    out = {"pairs": n, "read_len": L}
    for form in ("runs", "dist"):
        p = dict(W=64, O=33, text_stride_words=64, read_stride_words=64)
        prm = al._params(p)
        prm.reserved[1] = 1
        if form == "dist":
            al._check(al.lib.scrg_align_device_distance(al.h, C.byref(prm), b.n, *[api._ptr(x) for x in (b.seq, b.desc, b.ed, b.te, b.st)]))
        else:
            b.arena()
            al._check(al.lib.scrg_align_device(al.h, C.byref(prm), b.n, *[api._ptr(x) for x in (b.seq, b.desc, b.slices, b.ed, b.nr, b.st)]))
        b.torch.cuda.synchronize()
        s = al.debug_stats_lane()
        r = max(1, s["rounds"])
        out[form] = {"kernel_ms": al.last_kernel_ms(), "rounds": s["rounds"],
                     "cycles_per_round": {k: s["cycles_" + k] / r for k in ("fetch", "setup", "table", "traceback", "pass1")}}
        log("stats %-5s %.3f ms, cycles per round: %r" % (form, out[form]["kernel_ms"], {k: round(v) for k, v in out[form]["cycles_per_round"].items()}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True)
    ap.add_argument("--stats-lib", default=None)
    ap.add_argument("--extra-lib", default=None, help="an experimental build whose distance launch is timed as well (64/33 only)")
    ap.add_argument("--extra-waves", type=int, default=0, help="its waves_per_cu")
    ap.add_argument("--part", default="all", choices=["kernel", "other", "small", "host", "stats", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.launches >= 7 or args.scale < 1.0, "the median of at least 7 launches"
    als = {"parent": make_aligner(args.base_lib), "this": make_aligner(None)}
    als_x = dict(als, extra=make_aligner(args.extra_lib)) if args.extra_lib else als
    n10k, n150 = int(100_000 * args.scale), int(4_000_000 * args.scale)
    doc = {}
    if args.part in ("kernel", "all"):
        doc["kernel_100k_x_10kb_w64_o33"] = kernel_part(als_x, n10k, 10_000, 64, 33, args.launches, 1, args.extra_waves)
    if args.part in ("other", "all"):
        doc["kernel_100k_x_10kb_w256_o129"] = kernel_part(als, n10k, 10_000, 256, 129, args.launches, 1)
    if args.part in ("small", "all"):
        doc["kernel_4M_x_150bp_w64_o33"] = kernel_part(als, n150, 150, 64, 33, args.launches, 2)
    if args.part in ("host", "all"):
        doc["host_align_pairs_100k_x_10kb"] = host_part(als, n10k, 10_000, 3, 1)
    if args.part in ("stats", "all") and args.stats_lib:
        doc["phase_counters_w64_o33"] = stats_part(args.stats_lib, n10k, 10_000, 1)
    print(json.dumps(doc))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(doc)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
