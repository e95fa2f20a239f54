"""The pileup sites in numpy, from the rule's text in include/scrooge_amd.h (PILEUP SITES) — written apart from
scrooge_amd/csrc/site_rule.h, which the host twin and the kernels compile: the tests hold both to this, record for record."""
import numpy as np

DTYPE = np.dtype([("pos", np.uint64), ("counts", np.uint32, (7,)), ("ref", np.uint8), ("alt", np.uint8), ("call", np.uint8), ("flags", np.uint8)])
DEL, NONE = 4, 255
F_NONREF, F_INS, F_CALL = 1, 2, 4
CODES = {ord(ch): k for k, ch in enumerate("ACGT")}
CODES.update({ord(ch): k for k, ch in enumerate("acgt")})


def ref_codes(genome):
    """bytes / str -> uint8 codes (A0 C1 G2 T3, either case)"""
    raw = np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)
    table = np.full(256, 255, dtype=np.uint8)
    for ch, k in CODES.items():
        table[ch] = k
    out = table[raw]
    assert (out < 4).all(), "the model takes ACGTacgt only"
    return out


def sites(counts, ref, rule):
    """counts: (7, target_len + 1) uint32; ref: target_len codes; rule: (min_depth, min_alt, min_alt_per_mille) -> DTYPE records in
    ascending pos.  All arithmetic in Python-int-safe 64 bits: a count is below 2^32, a depth below 6 * 2^32, times 1000 below 2^45."""
    min_depth, min_alt, per_mille = (int(x) for x in rule)
    counts = np.asarray(counts, dtype=np.uint32)
    ref = np.asarray(ref, dtype=np.uint8)
    L = len(ref)
    assert counts.shape == (7, L + 1)
    c = counts[:, :L].astype(np.uint64)                  # slot target_len is never a site
    pos = np.arange(L)
    depth = c[0] + c[1] + c[2] + c[3] + c[4] + c[5]
    n = np.zeros((5, L), dtype=np.uint64)
    for b in range(4):
        n[b] = c[1 + b] + np.where(ref == b, c[0], np.uint64(0))
    n[4] = c[5]
    n_ref = n[ref, pos]
    nonref = depth - n_ref
    # alt: the b != r with the largest n[b], ties to the smallest b
    alt = np.full(L, NONE, dtype=np.int64)
    n_alt = np.zeros(L, dtype=np.uint64)
    for b in range(5):
        better = (ref != b) & ((alt == NONE) | (n[b] > n_alt))
        alt = np.where(better, b, alt)
        n_alt = np.where(better, n[b], n_alt)
    call = np.where(n_alt > n_ref, alt, ref.astype(np.int64))
    alt = np.where(nonref == 0, NONE, alt)

    def passes(x):
        return (x >= np.uint64(min_alt)) & (x * np.uint64(1000) >= np.uint64(per_mille) * depth)

    by_nonref, by_ins = passes(nonref), passes(c[6])
    is_site = (depth >= np.uint64(min_depth)) & (by_nonref | by_ins)
    flags = (np.where((nonref > 0) & by_nonref, F_NONREF, 0) | np.where((c[6] > 0) & by_ins, F_INS, 0) | np.where(call != ref, F_CALL, 0))
    at = np.nonzero(is_site)[0]
    out = np.zeros(len(at), dtype=DTYPE)
    out["pos"] = at
    out["counts"] = counts[:, at].T
    out["ref"] = ref[at]
    out["alt"] = alt[at]
    out["call"] = call[at]
    out["flags"] = flags[at]
    return out


def one(c, r, rule):
    """one position, in plain Python integers: (is_site, alt, call, flags) — the model's own cross-check"""
    min_depth, min_alt, per_mille = rule
    c = [int(x) for x in c]
    depth = sum(c[:6])
    n = [c[1 + b] + (c[0] if b == r else 0) for b in range(4)] + [c[5]]
    nonref = depth - n[r]
    alt = max((b for b in range(5) if b != r), key=lambda b: (n[b], -b))
    call = alt if n[alt] > n[r] else r
    if nonref == 0:
        alt = NONE

    def passes(x):
        return x >= min_alt and x * 1000 >= per_mille * depth

    site = depth >= min_depth and (passes(nonref) or passes(c[6]))
    flags = (F_NONREF if nonref > 0 and passes(nonref) else 0) | (F_INS if c[6] > 0 and passes(c[6]) else 0) | (F_CALL if call != r else 0)
    return site, alt, call, flags
