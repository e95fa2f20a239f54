"""Reversed texts (SCRG_TEXT_REVCOMP) and anchored alignment, measured on one GPU, in one process.

kernel  single launches on device buffers (lane-interleaved layout, one stream, runs output, scrg_last_kernel_ms), the median of
        --launches (>= 7), the forms ALTERNATING launch by launch so that they share the box's state.  Every pair's row holds
        its text, the reverse complement of its text, and its read, so that a flagged pair (text = the reverse complement of the
        second copy) is the SAME alignment problem as the forward pair, and every form must give the same distances:
            parent_fwd     all pairs forward, --base-lib (a library built from the parent commit)
            this_fwd       all pairs forward, this library, text strands off
            this_fwd_on    all pairs forward, text strands on (the uniform branch is tested, never taken)
            this_rev       all pairs text-reversed
            this_half      every second pair text-reversed
        for 100 000 x 10 kb ONT-error pairs at W/O = 64/33 and 256/129.
host    scrg_align_mapping_anchored against scrg_align_mapping_resident (start = anchor - read position: the start guess) on the
        same reads: 25 000 x 10 kb x 1 candidate and 1 M x 150 bp x 4, pairs per second, and the bytes each call moves over PCIe
        as the formats state them (H2D: the packed rows — a read is packed once per call by the resident call, each half of every
        candidate by the anchored one — plus 16 bytes of scalars per pair; D2H: 8 bytes per pair plus 2 per run).
edits   reads with an indel between their start and their anchor, 10 000 of them: the sum of the edits of the anchored
        alignment and of the alignment from the start guess.

    python3 tests/tools/bench_anchored.py --base-lib ab_libs/parent/libscrooge_amd.so [--part kernel|host|edits|all] [--scale 1.0]
                                          [--launches 7] [--out profiles/anchored.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from scrooge_amd import api, synth
from bench_distance import log, make_aligner, med

_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return b.translate(_RC)[::-1]


# ------------------------------------------------------------------------------------------------ kernel
class TwoWayBatch:
    """n pairs on the device, row p = text | reverse complement of the text | read (lane-interleaved groups of 64 rows)."""

    def __init__(self, al, n, L, seed):
        import torch
        self.torch, self.n = torch, n
        dev = torch.device("cuda", 0)
        rng = np.random.Generator(np.random.PCG64(seed))
        err, ratio = synth.PROFILES["ont"]
        base_n = min(n, 2048)                  # distinct pairs; the batch repeats them in a seeded order (the kernels cannot tell)
        pairs = [synth.make_pair(L, err, ratio, rng) for _ in range(base_n)]
        tw, rw = (max(len(t) for t, _ in pairs) + 31) // 32, (L + 31) // 32
        wpr = 2 * tw + rw
        rows = np.zeros((base_n, wpr * 32), dtype=np.uint8)
        tl = np.zeros(base_n, dtype=np.int64)
        for k, (t, q) in enumerate(pairs):
            rows[k, :len(t)] = synth.BASES[t]
            rows[k, tw * 32: tw * 32 + len(t)] = synth.BASES[3 - t[::-1]]
            rows[k, 2 * tw * 32: 2 * tw * 32 + len(q)] = synth.BASES[q]
            tl[k] = len(t)
        pick = rng.integers(0, base_n, n)
        al.set_stream(0)
        self.seq = torch.zeros(((n + 63) // 64) * 64 * wpr + api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        CH = 1 << 14                           # (whole groups of 64 rows at a time: the ASCII copy stays small)
        for a in range(0, n, CH):
            part = torch.from_numpy(rows[pick[a: a + CH]]).to(dev).view(-1)
            al.pack_planar_groups(part, min(CH, n - a), wpr, self.seq[(a // 64) * 64 * wpr:], bad)
        assert int(bad) == 0
        idx = np.arange(n, dtype=np.int64)
        self.cap = (2 * L + 16 + 15) // 16 * 16
        word = lambda w: 32 * (((idx // 64) * wpr + w) * 64 + idx % 64)
        tlen = tl[pick]

        def desc(rev_mask):
            t_off = np.where(rev_mask, word(tw) | np.int64(-2 ** 63), word(0))
            return torch.from_numpy(np.stack([t_off, tlen, word(2 * tw), np.full(n, L), idx * self.cap, np.full(n, self.cap)], axis=1).astype(np.int64)).to(dev)
        self.desc = {"fwd": desc(np.zeros(n, bool)), "rev": desc(np.ones(n, bool)), "half": desc(idx % 2 == 1)}
        self.ed = torch.empty(n, dtype=torch.int64, device=dev)
        self.st = torch.empty(n, dtype=torch.int32, device=dev)
        self.nr = torch.empty(n, dtype=torch.int32, device=dev)
        self.slices = torch.empty(n * self.cap * 2, dtype=torch.uint8, device=dev)


FORMS = [("parent_fwd", "parent", "fwd", False), ("this_fwd", "this", "fwd", False), ("this_fwd_on", "this", "fwd", True),
         ("this_rev", "this", "rev", True), ("this_half", "this", "half", True)]


def launch(als, b, form, W, O):
    name, who, which, on = form
    al = als[who]
    if who == "this":
        al.set_text_strands(on)
    al.align_device(b.n, b.seq, b.desc[which], b.slices, b.ed, b.nr, b.st, W=W, O=O, text_stride_words=64, read_stride_words=64)
    b.torch.cuda.synchronize()
    return al.last_kernel_ms()


def kernel_part(als, b, L, W, O, launches):
    n = b.n
    for al in als.values():
        al.set_stream(0)
    ref = None
    for f in FORMS:                                         # warm-up, and every form gives every pair the same distance
        launch(als, b, f, W, O)
        assert not bool(b.st.any()), f[0]
        if ref is None:
            ref = b.ed.clone()
        assert bool((b.ed == ref).all()), f[0]
    samples = {f[0]: [] for f in FORMS}
    for _ in range(launches):
        for f in FORMS:
            samples[f[0]].append(launch(als, b, f, W, O))
    als["this"].set_text_strands(False)
    out = {"pairs": n, "read_len": L, "W": W, "O": O, "launches": launches}
    for name, a in samples.items():
        out[name] = {"align_ms_median": med(a), "align_ms_all": [round(x, 4) for x in a], "align_ms_spread": (max(a) - min(a)) / med(a)}
    p = out["parent_fwd"]["align_ms_median"]
    for name in samples:
        if name != "parent_fwd":
            out[name + "_over_parent_fwd"] = out[name]["align_ms_median"] / p
    log("%d x %d bp at %d/%d: " % (n, L, W, O) + ", ".join("%s %.3f ms" % (k, out[k]["align_ms_median"]) for k in samples))
    return out


# ------------------------------------------------------------------------------------------------ host
def seeded_reads(genome, n_base, L, rng, indel=False):
    """n_base reads: a genome stretch with ONT-profile edits around 12 bases copied exactly -> (read, anchor genome, anchor read).
    indel: two extra bases between the read's start and its anchor (the start guess anchor - read position is then off by two)."""
    out = []
    code = np.searchsorted(synth.BASES, np.frombuffer(genome, dtype=np.uint8)).astype(np.uint8)
    err, ratio = synth.PROFILES["ont"]
    for _ in range(n_base):
        ga = int(rng.integers(L, len(genome) - L - 64))
        la = L // 2
        left = synth.BASES[synth.mutate(code[ga - la: ga], err, ratio, rng)].tobytes()
        if indel:
            left = left[: len(left) // 2] + b"TT" + left[len(left) // 2:]
        right = genome[ga: ga + 12] + synth.BASES[synth.mutate(code[ga + 12: ga + L - la], err, ratio, rng)].tobytes()
        out.append((left + right, ga, len(left)))
    return out


def host_part(al, n, L, n_cand, passes, seed, genome_len=4_000_000):
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = synth.random_seq(genome_len, rng)
    al.use_own_stream()
    al.set_genome(genome)
    base = seeded_reads(genome, min(n, 2048), L, rng)
    pick = rng.integers(0, len(base), n)
    reads = [base[k][0] for k in pick]
    anchors, starts = [], []
    for k in pick:
        _, ga, ra = base[k]
        others = [(int(rng.integers(ra, genome_len - L)), ra) for _ in range(n_cand - 1)]
        anchors.append([(ga, ra)] + others)
        starts.append([g - r for g, r in anchors[-1]])
    rw = lambda ln: 8 * ((ln + 31) // 32)
    out = {"reads": n, "read_len": L, "candidates_per_read": n_cand, "pairs": n * n_cand, "passes": passes}
    for name in ("resident", "anchored"):
        ms = []
        for _ in range(passes + 1):                         # (the first pass warms the buffers up)
            if name == "resident":
                r = al.align_mapping(None, reads, starts, arrays=True, outputs=api.SCRG_OUT_RUNS)
            else:
                r = al.align_anchored(reads, anchors, arrays=True, outputs=api.SCRG_OUT_RUNS)
            ms.append(al.last_timing["total_ns"] / 1e6)
        tot = med(ms[1:])
        n_runs = int(r["run_offset"][-1])
        pairs = n * n_cand
        if name == "resident":       # a read's row once; 16 bytes of scalars per pair
            h2d = sum(rw(len(x)) for x in reads) + 16 * pairs
            d2h = 8 * pairs + 2 * n_runs
        else:                        # both halves of every candidate are rows of their own, and pairs of their own on the wire
            h2d = sum(rw(ra) + rw(len(x) - ra) for x, a in zip(reads, anchors) for _, ra in a) + 32 * pairs
            d2h = 16 * pairs + 2 * n_runs
        out[name] = {"total_ms_median": tot, "pairs_per_s": pairs / tot * 1e3, "h2d_bytes_lower_bound": int(h2d), "d2h_bytes": int(d2h),
                     "edits_sum": int(r["edit_distance"].sum())}
        log("host %-9s %d x %d bp x %d: %.1f ms per call, %.3f M pairs/s, >= %.1f MB up, %.1f MB down"
            % (name, n, L, n_cand, tot, pairs / tot / 1e3, h2d / 1e6, d2h / 1e6))
    out["anchored_over_resident_pairs_per_s"] = out["anchored"]["pairs_per_s"] / out["resident"]["pairs_per_s"]
    out["note"] = ("h2d: rows are padded to their chunk's longest read, so the figure is a lower bound; the C entry points are given the same Python lists, "
                   "whose marshalling is outside total_ns")
    return out


def edits_part(al, n, L, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = synth.random_seq(1_000_000, rng)
    al.use_own_stream()
    al.set_genome(genome)
    base = seeded_reads(genome, n, L, rng, indel=True)
    reads = [x[0] for x in base]
    anchored = al.align_anchored(reads, [[(ga, ra)] for _, ga, ra in base], arrays=True, outputs=api.SCRG_OUT_DISTANCE)
    guess = al.align_mapping(None, reads, [[ga - ra] for _, ga, ra in base], arrays=True, distance_only=True)
    out = {"reads": n, "read_len": L, "edits_anchored": int(anchored["edit_distance"].sum()), "edits_start_guess": int(guess["edit_distance"].sum()),
           "reads_with_fewer_edits_anchored": int((anchored["edit_distance"] < guess["edit_distance"]).sum()),
           "reads_with_more_edits_anchored": int((anchored["edit_distance"] > guess["edit_distance"]).sum())}
    log("edits: anchored %d, start guess %d over %d reads" % (out["edits_anchored"], out["edits_start_guess"], n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None, help="a library built from the parent commit (the kernel part needs it)")
    ap.add_argument("--part", default="all", choices=["kernel", "kernel64", "kernel256", "host", "edits", "all"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.launches >= 7 or args.scale < 1.0, "the median of at least 7 launches"
    doc = {"command": " ".join(["python3", "tests/tools/bench_anchored.py"] + sys.argv[1:])}
    this = make_aligner(None)
    if args.part in ("kernel", "kernel64", "kernel256", "all"):
        assert args.base_lib, "--base-lib"
        als = {"parent": make_aligner(args.base_lib), "this": this}
        b = TwoWayBatch(this, int(100_000 * args.scale), 10_000, 1)
        if args.part != "kernel256":
            doc["kernel_100k_x_10kb_w64_o33"] = kernel_part(als, b, 10_000, 64, 33, args.launches)
        if args.part != "kernel64":
            doc["kernel_100k_x_10kb_w256_o129"] = kernel_part(als, b, 10_000, 256, 129, args.launches)
        del b
    if args.part in ("host", "all"):
        doc["host_25k_x_10kb_x_1"] = host_part(this, int(25_000 * args.scale), 10_000, 1, 3, 3)
        doc["host_1M_x_150bp_x_4"] = host_part(this, int(1_000_000 * args.scale), 150, 4, 2, 4)
    if args.part in ("edits", "all"):
        doc["edits_saved_10k_reads"] = edits_part(this, int(10_000 * args.scale), 400, 5)
    print(json.dumps(doc))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        cmds = old.get("commands", [])
        cmds.append(doc.pop("command"))
        old.update(doc)
        old["commands"] = cmds
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
