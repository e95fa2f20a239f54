#!/usr/bin/env python3
"""reference_random.json: the answers of the UNMODIFIED reference CPU path (oracle/_ref/libgenasm_ref.so, default knobs W=64 O=33)
for the seeded inputs of tests/test_oracle.py::test_oracle_matches_reference_build_random, so that the test holds the oracle to
them where the reference build is absent.  Runs only where oracle/_ref was built; the fixture is data: the (edit distance, CIGAR)
the reference returned for every pair, in the order the test generates the pairs."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.pyoracle import Reference  # noqa: E402
from tests.test_oracle import reference_random_inputs  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    T, Q = reference_random_inputs()
    eds, cigars, _ = Reference().align(T, Q)
    with open(os.path.join(HERE, "reference_random.json"), "w") as f:
        json.dump({"knobs": {"W": 64, "O": 33}, "pairs": len(T), "edit_distances": eds, "cigars": cigars}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
