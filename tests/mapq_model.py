"""The read summary and its MAPQ (include/scrooge_amd.h: READ SUMMARY AND MAPPING QUALITY) restated in plain Python, one read and one
candidate at a time, from the rule's text: what the tests hold the host twin, the kernel and the host path to."""

HAS_WINNER, TIED, HAS_SECOND, KEPT = 1, 2, 4, 8
NONE = 0xffffffffffffffff
NO_ED = 0xffffffff
DEFAULT_RULE = (10, 60, 250, 0)          # per_edit, max_q, zero_per_mille, min_keep_q


def mapq(rule, read_len, has_winner, n_tied, best_ed, second_ed):
    """second_ed: None when there is no second."""
    per_edit, max_q, zero_per_mille, _ = rule
    if not has_winner or n_tied > 1:
        return 0
    cap = max_q
    if read_len != 0:
        cap = max_q - min(max_q, (max_q * 1000 * best_ed) // (zero_per_mille * read_len))
    if second_ed is None:
        return cap
    return min(cap, min(max_q, per_edit * (second_ed - best_ed)))


def summarise(rule, read_len, eds, eligible, first=0):
    """One read: eds[c] and eligible[c] per candidate, `first` the pair index of candidate 0.
    -> dict(winner, best_ed, second_ed, n_tied, n_eligible, n_candidates, mapq, flags)."""
    winner = None
    for c, (e, ok) in enumerate(zip(eds, eligible)):
        if ok and (winner is None or e < eds[winner]):
            winner = c
    n_eligible = sum(1 for ok in eligible if ok)
    if winner is None:
        return dict(winner=NONE, best_ed=NO_ED, second_ed=NO_ED, n_tied=0, n_eligible=n_eligible, n_candidates=len(eds), mapq=0, flags=0)
    best = eds[winner]
    n_tied = sum(1 for e, ok in zip(eds, eligible) if ok and e == best)
    above = [e for e, ok in zip(eds, eligible) if ok and e > best]
    second = min(above) if above else None
    q = mapq(rule, read_len, True, n_tied, best, second)
    flags = HAS_WINNER | (TIED if n_tied > 1 else 0) | (HAS_SECOND if second is not None else 0) | (KEPT if q >= rule[3] else 0)
    return dict(winner=first + winner, best_ed=best, second_ed=NO_ED if second is None else second, n_tied=n_tied, n_eligible=n_eligible,
                n_candidates=len(eds), mapq=q, flags=flags)


def summarise_all(rule, first, read_len, eds, eligible):
    """A batch: first[r] .. first[r + 1] are read r's pairs; read_len, eds and eligible per pair.  -> a list of summarise()'s dicts."""
    out = []
    for r in range(len(first) - 1):
        a, e = first[r], first[r + 1]
        out.append(summarise(rule, read_len[a] if e > a else 0, list(eds[a:e]), list(eligible[a:e]), a))
    return out


def keep_status(records, first, status, done=0, not_best=3):
    """The statuses with every `done` pair that is not the winner of a KEPT read as `not_best`."""
    out = list(status)
    for r, rec in enumerate(records):
        for p in range(first[r], first[r + 1]):
            if out[p] == done and not (rec["flags"] & KEPT and rec["winner"] == p):
                out[p] = not_best
    return out


def as_tuple(rec):
    return tuple(int(rec[k]) for k in ("winner", "best_ed", "second_ed", "n_tied", "n_eligible", "n_candidates", "mapq", "flags"))
