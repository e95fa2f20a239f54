"""The edit limit (scrg_ctx_set_edit_limit) at the device layer: the same seeded batch aligned with no limit and with one, in one
process, kernel time of each (interleaved, median of --reps), and the full-size checks:
  - every pair within the limit is identical to the no-limit run (edit distance, run count, status, its runs),
  - the pairs over the limit are exactly those whose no-limit edit distance exceeds the limit,
  - the edit distance reported for them lies in (limit, full edit distance] and they have no runs,
  - a sample of pairs matches the oracle through the window-end model (tests/test_edit_limit.py).
Workloads: (A) BASELINE configs[2]'s shape — 1 M x 150 bp reads x 4 candidates (true locus, two shifted, one random; the
generator of tests/tools/bench_mapping.py), max_edits = 15; (B) 25 k x 10 kb ONT reads x 4 candidates (the true text and three
unrelated ones), per_mille = 150; (C) BASELINE configs[1] — 100 k true 10 kb ONT pairs, per_mille = 150 (nothing should go over:
this prices the check); (D) 100 k reads as in (B), a queue deeper than the GPU has lanes (262 k): at the sizes of (B) and (C)
every lane gets ONE pair at the start, so a lane freed early finds nothing left to take.

    python3 tests/tools/bench_edit_limit.py [--out profiles/edit_limit.json] [--scale 1.0] [--sample 20000] [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import scrooge_amd
from scrooge_amd import api, synth
from oracle.pyoracle import Oracle
from bench_legs import device_pairs
from tests.test_edit_limit import window_model

DEV = torch.device("cuda", 0)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def mapping_150(n_reads, G=100_000_000, seed=42):
    """tests/tools/bench_mapping.py's generator (configs[2]): one random chromosome, reads of 150 bp with ~1 % errors (90:5:5)
    from random loci, candidates = true locus, one shifted left, one shifted right, one random locus."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gcodes = rng.integers(0, 4, G, dtype=np.uint8)
    genome = synth.BASES[gcodes]
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
    rnd = rng.integers(0, G - 10, n_reads)
    cands = np.stack([starts, sh1, sh2, rnd], axis=1)
    return genome, synth.BASES[reads], cands


def stage_mapping(al, genome, reads, cands):
    """Genome + read rows in one contiguous planar array; one descriptor per candidate (the genome suffix at its start)."""
    G, (nr, L) = genome.size, reads.shape
    gw, rw = (G + 31) // 32, (L + 31) // 32
    ascii_ = torch.zeros((gw + nr * rw) * 32, dtype=torch.uint8, device=DEV)
    ascii_[:G] = torch.from_numpy(genome).to(DEV)
    rows = np.zeros((nr, rw * 32), dtype=np.uint8)
    rows[:, :L] = reads
    ascii_[gw * 32:] = torch.from_numpy(rows).to(DEV).view(-1)
    seq = torch.zeros(gw + nr * rw + api.SEQ_PAD_WORDS, dtype=torch.int64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    al.pack_planar(ascii_, seq, bad)
    torch.cuda.synchronize()
    assert int(bad) == 0
    del ascii_
    n = cands.size
    cap = (2 * L + 8 + 15) // 16 * 16
    st = torch.from_numpy(cands.reshape(-1).astype(np.int64)).to(DEV)
    r = torch.arange(nr, dtype=torch.int64, device=DEV).repeat_interleave(cands.shape[1])
    k = torch.arange(n, dtype=torch.int64, device=DEV)
    desc = torch.stack([st, G - st, (gw + r * rw) * 32, torch.full_like(k, L), k * cap, torch.full_like(k, cap)], dim=1).contiguous()
    host = {"genome": genome, "reads": reads, "cands": cands, "L": L}
    return seq, desc, cap, {}, host


def stage_rows(al, n_reads, L, n_cand, seed):
    """device_pairs (bench.py's generator) in lane-interleaved groups; candidate 0 of read r is its own text, the others the
    texts of other, random rows (unrelated random sequence)."""
    err, ratio = synth.PROFILES["ont"]
    rows, tw, rw, text_len = device_pairs(torch, n_reads, L, err, ratio, seed, DEV)
    wpr, Gp = tw + rw, api.GROUP
    seq = torch.zeros((n_reads + Gp - 1) // Gp * Gp * wpr + api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    al.pack_planar_groups(rows.view(-1), n_reads, wpr, seq, bad)
    torch.cuda.synchronize()
    assert int(bad) == 0
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 1)
    r = torch.arange(n_reads, dtype=torch.int64, device=DEV).repeat_interleave(n_cand)
    trow = r.clone()
    if n_cand > 1:
        other = torch.randint(0, n_reads, (n_reads, n_cand - 1), generator=g, device=DEV)
        trow.view(n_reads, n_cand)[:, 1:] = other
    first = lambda q: (q // Gp) * wpr * Gp + q % Gp
    n = n_reads * n_cand
    cap = (2 * L + 8 + 15) // 16 * 16
    k = torch.arange(n, dtype=torch.int64, device=DEV)
    desc = torch.stack([first(trow) * 32, torch.full_like(k, text_len), (first(r) + tw * Gp) * 32, torch.full_like(k, L),
                        k * cap, torch.full_like(k, cap)], dim=1).contiguous()
    host = {"rows": rows, "tw": tw, "trow": trow, "r": r, "text_len": text_len, "L": L}
    return seq, desc, cap, {"text_stride_words": Gp, "read_stride_words": Gp}, host


def sample_pairs(host, idx):
    """ASCII texts and reads of the sampled pairs (for the oracle)."""
    L = host["L"]
    if "genome" in host:
        g, reads, cands = host["genome"], host["reads"], host["cands"].reshape(-1)
        nc = host["cands"].shape[1]
        texts = [g[int(cands[k]): int(cands[k]) + 2 * L + 64].tobytes() for k in idx]
        rds = [reads[int(k) // nc].tobytes() for k in idx]
        return texts, rds
    rows, tw = host["rows"], host["tw"]
    tr, rr = host["trow"][torch.as_tensor(idx, device=DEV)], host["r"][torch.as_tensor(idx, device=DEV)]
    t = rows[tr][:, :host["text_len"]].cpu().numpy()
    q = rows[rr][:, tw * 32: tw * 32 + L].cpu().numpy()
    return [x.tobytes() for x in t], [x.tobytes() for x in q]


def run(al, seq, desc, cap, kw, runs, max_edits, per_mille):
    n = desc.shape[0]
    out = dict(ed=torch.empty(n, dtype=torch.int64, device=DEV), n_runs=torch.empty(n, dtype=torch.int32, device=DEV),
               status=torch.empty(n, dtype=torch.int32, device=DEV))
    runs.zero_()
    torch.cuda.synchronize()
    al.align_device(n, seq, desc, runs, out["ed"], out["n_runs"], out["status"], max_edits=max_edits,
                    max_edit_per_mille=per_mille, **kw)
    ms = al.last_kernel_ms()
    return ms, out


def workload(al, oracle, name, staged, max_edits, per_mille, reps, sample, threads):
    seq, desc, cap, kw, host = staged
    n = desc.shape[0]
    log("[%s] %d pairs staged" % (name, n))
    runs0 = torch.empty(n * cap * 2, dtype=torch.uint8, device=DEV)
    runs1 = torch.empty(n * cap * 2, dtype=torch.uint8, device=DEV)
    run(al, seq, desc, cap, kw, runs0, None, None)            # warm-up
    t_off, t_on = [], []
    for rep in range(reps):
        ms, out0 = run(al, seq, desc, cap, kw, runs0, None, None)
        t_off.append(ms)
        ms, out1 = run(al, seq, desc, cap, kw, runs1, max_edits, per_mille)
        t_on.append(ms)
        log("[%s] rep %d: no limit %.3f ms, limit %.3f ms" % (name, rep, t_off[-1], t_on[-1]))
    # ---- full-size checks (the last pair of runs)
    L = desc[:, 3]
    lim = torch.full_like(L, 1 << 62)
    if max_edits is not None:
        lim = torch.minimum(lim, torch.full_like(L, max_edits))
    if per_mille is not None:
        lim = torch.minimum(lim, per_mille * L // 1000)
    over = out1["status"] == api.DEVICE_STATUS_OVER_EDIT_LIMIT
    within = ~over
    checks = {
        "over_set_equals_full_ed_above_limit": bool(torch.equal(over, out0["ed"] > lim)),
        "within_identical_ed_nruns_status": bool(torch.equal(out0["ed"][within], out1["ed"][within]) and
                                                 torch.equal(out0["n_runs"][within], out1["n_runs"][within]) and
                                                 torch.equal(out0["status"][within], out1["status"][within])),
        "over_ed_in_limit_to_full_ed": bool(((out1["ed"][over] > lim[over]) & (out1["ed"][over] <= out0["ed"][over])).all()),
        "over_no_runs": bool((out1["n_runs"][over] == 0).all()),
    }
    # the runs of a pair: its first n_runs runs (past them a slice holds whatever the lane's ring held: unspecified)
    same = True
    r0, r1 = runs0.view(n, cap * 2), runs1.view(n, cap * 2)
    col = torch.arange(cap * 2, device=DEV)[None, :]
    for b in range(0, n, 16384):
        e = min(n, b + 16384)
        used = col < 2 * out0["n_runs"][b:e, None].long()
        diff = ((r0[b:e] != r1[b:e]) & used).any(dim=1) & within[b:e]
        same &= not bool(diff.any())
    checks["within_runs_identical"] = same
    # ---- sample vs the oracle, through the window-end model
    rng = np.random.Generator(np.random.PCG64(1234))
    idx = np.sort(rng.choice(n, size=min(sample, n), replace=False))
    texts, reads = sample_pairs(host, idx)
    t0 = time.time()
    eds, cigars, _, _ = oracle.align(texts, reads, threads=threads)
    log("[%s] oracle on %d pairs: %.1f s" % (name, len(idx), time.time() - t0))
    ed1, st1, nr1 = out1["ed"].cpu().numpy(), out1["status"].cpu().numpy(), out1["n_runs"].cpu().numpy()
    lim_h = lim.cpu().numpy()
    bad = 0
    for j, k in enumerate(idx):
        lk = int(lim_h[k]) if lim_h[k] < (1 << 62) else None
        m_over, m_ed = window_model(cigars[j], lk)
        if m_over:
            ok = st1[k] == api.DEVICE_STATUS_OVER_EDIT_LIMIT and ed1[k] == m_ed
        else:
            b = r1[k, :2 * int(nr1[k])].cpu().numpy().tobytes()
            got = "".join("%d%s" % (b[2 * q], chr(b[2 * q + 1])) for q in range(len(b) // 2))
            ok = st1[k] == 0 and ed1[k] == eds[j] and got == cigars[j]
        bad += 0 if ok else 1
    checks["oracle_sample_pairs"] = int(len(idx))
    checks["oracle_sample_matches"] = bad == 0
    med_off, med_on = float(np.median(t_off)), float(np.median(t_on))
    res = {"pairs": int(n), "limit": {"max_edits": max_edits, "per_mille": per_mille},
           "kernel_ms_no_limit": [round(x, 4) for x in t_off], "kernel_ms_limit": [round(x, 4) for x in t_on],
           "pairs_per_s_no_limit": n / (med_off / 1e3), "pairs_per_s_limit": n / (med_on / 1e3),
           "speedup": med_off / med_on, "share_over_limit": float(over.float().mean()), "checks": checks,
           "all_checks_pass": all(v for k, v in checks.items() if isinstance(v, bool))}
    log("[%s] %.2f M -> %.2f M pairs/s (x%.3f), %.1f %% over the limit, checks %s" % (
        name, res["pairs_per_s_no_limit"] / 1e6, res["pairs_per_s_limit"] / 1e6, res["speedup"], 100 * res["share_over_limit"],
        "pass" if res["all_checks_pass"] else "FAIL %r" % checks))
    del runs0, runs1
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_limit.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the full sizes (a quick look; the profile is full size)")
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="oracle threads")
    ap.add_argument("--only", default="ABCD")
    args = ap.parse_args()
    al = scrooge_amd.Aligner(0)
    al.set_stream(0)
    oracle = Oracle()
    s = args.scale
    out = {"tool": "tests/tools/bench_edit_limit.py", "layer": "device (scrg_align_device, runs output, W=64 O=33)",
           "scale": s, "device": torch.cuda.get_device_name(0)}
    if "A" in args.only:
        g, rd, cd = mapping_150(int(1_000_000 * s))
        out["A_mapping_150bp_x4_max_edits_15"] = workload(al, oracle, "A", stage_mapping(al, g, rd, cd), 15, None, args.reps, args.sample, args.threads)
        del g, rd, cd
    if "B" in args.only:
        out["B_ont_10kb_x4_1true_3random_per_mille_150"] = workload(al, oracle, "B", stage_rows(al, int(25_000 * s), 10_000, 4, 5),
                                                                      None, 150, args.reps, args.sample, args.threads)
    if "D" in args.only:
        out["D_ont_10kb_x4_deep_queue_per_mille_150"] = workload(al, oracle, "D", stage_rows(al, int(100_000 * s), 10_000, 4, 9),
                                                                   None, 150, args.reps, args.sample, args.threads)
    if "C" in args.only:
        out["C_ont_10kb_true_pairs_per_mille_150"] = workload(al, oracle, "C", stage_rows(al, int(100_000 * s), 10_000, 1, 7),
                                                                None, 150, args.reps, args.sample, args.threads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v["speedup"], v["share_over_limit"], v["all_checks_pass"]) if isinstance(v, dict) else v
                      for k, v in out.items()}))


if __name__ == "__main__":
    main()
