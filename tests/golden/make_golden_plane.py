#!/usr/bin/env python3
"""Fixtures plane_wW_oO.json: the answers of the UNMODIFIED reference CPU path, built by oracle/Makefile at every setting of
tests/plane_inputs.py:SETTINGS, on the input set plane_inputs(W, O) — never the oracle's, never a GPU result.

A fixture stores results, not sequences (the tests regenerate the inputs and compare `inputs_sha256` first): W, O, the pair
count, the group of every pair (run-length coded), every edit distance and every CIGAR — in full for the lattice and degenerate
groups and wherever it is at most CIGAR_TEXT_LIMIT characters, else '#' + 16 hex digits of its sha256; an entry '^' repeats
the one before.  The settings of
MAPPING_SETTINGS also carry the answers of the mapping-shaped call (mapping_inputs: a pair's text is the genome's suffix), from
the reference's own align_mapping.  Runs only where oracle/_ref/ holds the reference builds (`make -C oracle ref`)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Reference  # noqa: E402
from tests import plane_inputs as pi  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def make(W, O):
    t, q, g = pi.plane_inputs(W, O)
    ref = Reference(W, O)
    eds, cigars, _ = ref.align(t, q, threads=8)
    runs = []
    for name in g:
        if runs and runs[-1][0] == name:
            runs[-1][1] += 1
        else:
            runs.append([name, 1])
    out = {"W": W, "O": O, "n": len(t), "inputs_sha256": pi.inputs_digest(t, q, g), "groups": runs, "ed": eds,
           "cigar": pi.pack_cigars(cigars, g)}
    if (W, O) in pi.MAPPING_SETTINGS:
        genome, reads, cands = pi.mapping_inputs(W, O)
        m_eds, m_cigars, _ = ref.align_mapping(genome, reads, cands, threads=8)
        out["mapping"] = {"ed": m_eds, "cigar": pi.pack_cigars(m_cigars, ["mapping"] * len(m_cigars))}
    return out


def main():
    total = 0
    for W, O in pi.SETTINGS:
        out = make(W, O)
        path = os.path.join(HERE, pi.fixture_name(W, O))
        with open(path, "w") as f:
            json.dump(out, f, separators=(",", ":"))
            f.write("\n")
        size = os.path.getsize(path)
        total += size
        print("W=%d O=%d pairs %d, mean ed %.1f, %d bytes%s" % (W, O, out["n"], sum(out["ed"]) / out["n"], size,
                                                              ", + mapping" if "mapping" in out else ""))
    print("%d fixtures, %d bytes" % (len(pi.SETTINGS), total))


if __name__ == "__main__":
    main()
