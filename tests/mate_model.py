"""The paired-end rule (include/scrooge_amd.h, MATE PAIRS) in plain Python integers, written from its text: what the host twin
scrg_mates_from_distances and the kernel behind scrg_select_mates are held to.  No numpy, no library."""

FR, RF, FF, ANY = 0, 1, 2, 3
PROPER, HAS_A, HAS_B, TIED = 1, 2, 4, 8
NONE64, NONE32 = 2 ** 64 - 1, 2 ** 32 - 1
OVER_LIMIT = 7            # SCRG_PAIR_OVER_EDIT_LIMIT


def span_of(s_a, len_a, s_b, len_b):
    return max(s_a + len_a, s_b + len_b) - min(s_a, s_b)


def oriented(orientation, s_a, r_a, s_b, r_b):
    if orientation == ANY:
        return True
    if orientation == FF:
        return r_a == r_b
    if r_a == r_b:
        return False
    fwd, rev = (s_a, s_b) if r_b else (s_b, s_a)
    return fwd <= rev if orientation == FR else rev <= fwd


def best_of(eds, eligible):
    """best-candidate mode's rule -> (index or None, whether another eligible candidate shares the winner's distance)"""
    ok = [k for k in range(len(eds)) if eligible[k]]
    if not ok:
        return None, False
    w = min(ok, key=lambda k: (eds[k], k))
    return w, sum(1 for k in ok if eds[k] == eds[w]) > 1


def choose(rule, side_a, side_b):
    """rule: (min_span, max_span, orientation, penalty); a side: (starts, reverses, eds, eligibles, read_len).
    -> dict with the record's fields (winner: indices within the sides, None: none) and the sides' 0/1 winner marks."""
    lo, hi, orientation, penalty = rule
    s_a, r_a, e_a, ok_a, len_a = side_a
    s_b, r_b, e_b, ok_b, len_b = side_b
    proper = []
    for i in range(len(s_a)):
        for j in range(len(s_b)):
            if ok_a[i] and ok_b[j] and oriented(orientation, s_a[i], r_a[i], s_b[j], r_b[j]) and lo <= span_of(s_a[i], len_a, s_b[j], len_b) <= hi:
                proper.append((e_a[i] + e_b[j], i, j))
    proper.sort()
    a, tie_a = best_of(e_a, ok_a)
    b, tie_b = best_of(e_b, ok_b)
    rec = {"second_cost": NONE32, "n_proper": min(len(proper), 65535)}
    if proper and proper[0][0] <= e_a[a] + e_b[b] + penalty:
        cost, wa, wb = proper[0]
        rec["flags"] = PROPER | HAS_A | HAS_B
        if len(proper) > 1:
            rec["second_cost"] = proper[1][0]
            if proper[1][0] == cost:
                rec["flags"] |= TIED
    else:
        wa, wb = a, b
        cost = (e_a[a] if a is not None else 0) + (e_b[b] if b is not None else 0)
        rec["flags"] = (HAS_A if a is not None else 0) | (HAS_B if b is not None else 0) | (TIED if tie_a or tie_b else 0)
    rec["winner"] = (wa, wb)
    rec["cost"] = cost
    rec["span"] = min(span_of(s_a[wa], len_a, s_b[wb], len_b), NONE32) if wa is not None and wb is not None else 0
    rec["is_best_a"] = [1 if k == wa else 0 for k in range(len(s_a))]
    rec["is_best_b"] = [1 if k == wb else 0 for k in range(len(s_b))]
    return rec
