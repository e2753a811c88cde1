#!/usr/bin/env python3
"""Prints the truth census the CPU tests assert (tests/test_geno_host.py: CENSUS): a diploid sample over the generated genome of lift_model -
per IUPAC site a genotype drawn among the code's members, per bubble R/R, R/V or V/V, error-free reads from both haplotypes on both strands -
mapped without a GPU (the oracle's `align -n 3 -o 1`, the models' records, `places2sam -B t -J -R -a 1 -w 5 -G`), and its calls compared with
the drawn genotypes: how many entries are called, how many with GQ >= 20, and how many of those disagree - each disagreement is printed.

usage: python tools/geno_generated_reference.py   (needs the built tools: make -C bwbble_amd && make -C oracle)"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import geno_model  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        m = geno_model.build_chain(d)
        figures, wrong = geno_model.census(m)
        print("reads", len(m.sample.reads))
        print("CENSUS =", figures)
        for w in wrong:
            print("disagreement:", w)
