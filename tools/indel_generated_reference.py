#!/usr/bin/env python3
"""Where the REFERENCE's own `index` + `align -n 3 -o 1` + `aln2sam` place the reads of tests/indel_model.py on the generated multi-genome of
tests/lift_model.py, on the CPU: the census behind tests/test_indel_host.py - every error-free read that the name judge calls clean for some
bubble must lie on the record it was cut from, at its offset, ungapped; no exception is allowed.
usage: tools/indel_generated_reference.py <a bwbble binary built from the reference> [work directory]"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_indel_host  # noqa: E402


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        work = sys.argv[2] if len(sys.argv) > 2 else tmp
        os.makedirs(work, exist_ok=True)
        print("  ".join(f"{k} {v}" for k, v in test_indel_host.census(sys.argv[1], work).items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
