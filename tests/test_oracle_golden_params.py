"""Pins the CPU oracle to the REAL reference with max_best and no_indel_length away from their defaults: the fixtures of
tests/golden/make_golden_params.py (the reference's align_reads_inexact, driven through a harness - `bwbble align` has no flag for either
field).  CPU only; the reference is not needed here."""
import os

import pytest

import oracle_lib
from golden.make_golden_params import CONFIGS, fixture_bytes


def run(oracle, golden, tmp_path, fa, fq, flags, **fields):
    out = str(tmp_path / "o.aln")
    oracle.align_fastq(os.path.join(golden, fa + ".bwt"), os.path.join(golden, fq), out, oracle.params(flags, **fields))
    return open(out, "rb").read()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_aln_bytes_match_reference_at_non_default_fields(oracle, golden, tmp_path, name):
    fa, fq, flags, fields, _ = CONFIGS[name]
    assert run(oracle, golden, tmp_path, fa, fq, flags, **fields) == fixture_bytes(name)


def test_the_fixtures_cover_what_was_asked_and_decide_something(golden):
    """max_best 0, 1, 3 with -n 3; no_indel_length 0, 2, 12, 60; a negative value of each; -o 2 -e 3 with no_indel_length 1 and 2 - and the
    REFERENCE's records change with either field: every fixture differs from the default-valued fixture of the same reads and flags, or from
    the fixture of a neighbouring value, and every no_indel_length fixture below half a read holds gapped hits"""
    cfg = list(CONFIGS.values())
    assert {0, 1, 3} <= {c[3].get("max_best") for c in cfg if c[2] == ["-n", "3"]}
    assert {0, 2, 12, 60} <= {c[3].get("no_indel_length") for c in cfg}
    assert any(c[3].get("max_best", 0) < 0 for c in cfg) and any(c[3].get("no_indel_length", 0) < 0 for c in cfg)
    assert {1, 2} <= {c[3].get("no_indel_length") for c in cfg if c[2][2:] == ["-o", "2", "-e", "3"]}
    hits = lambda data: oracle_lib.parse_aln(data)
    differ = lambda a, b: sum(x != y for x, y in zip(hits(a), hits(b)))
    default = lambda name: open(os.path.join(golden, name), "rb").read()
    # against the default-valued run of the same reads with the same flags
    assert [differ(fixture_bytes(n), default("rep_n3.aln")) for n in ("rep_mb0", "rep_mb1", "rep_mb3")] == [40, 20, 0]
    assert [differ(fixture_bytes(n), default("rep_gap_n4.aln")) for n in ("repgap_mbneg", "repgap_mb0", "repgap_mb1", "repgap_mb3", "repgap_nil60")] == [28, 28, 16, 4, 40]
    assert [differ(fixture_bytes(n), default("toy_n3.aln")) for n in ("toy_nilneg", "toy_nil0", "toy_nil2", "toy_nil3", "toy_nil12")] == [1, 1, 1, 1, 2]
    assert [differ(fixture_bytes(n), default("gapo_o5.aln")) for n in ("gapo_o5e2_nil8", "gapo_o5e2_nil12")] == [2, 5]
    # against the neighbouring value: the negative value, 0 and 2 on the one side, 3 and 12 on the other; with two gap opens every step
    chain = ["toy_nilneg", "toy_nil0", "toy_nil2", "toy_nil3", "toy_nil12"]
    assert [differ(fixture_bytes(a), fixture_bytes(b)) for a, b in zip(chain, chain[1:])] == [1, 0, 1, 3]
    chain = ["toy_o2e3_nilneg", "toy_o2e3_nil0", "toy_o2e3_nil1", "toy_o2e3_nil2", "toy_o2e3_nil3"]
    assert all(differ(fixture_bytes(a), fixture_bytes(b)) >= 1 for a, b in zip(chain, chain[1:]))
    assert differ(fixture_bytes("toy_o2e3_mb0_nil2"), fixture_bytes("toy_o2e3_nil2")) >= 1
    for name, c in CONFIGS.items():
        if "no_indel_length" in c[3]:
            gapped = sum(1 for r in hits(fixture_bytes(name)) for h in r if h["gapo"])
            assert (gapped == 0) if c[3]["no_indel_length"] == 60 else (gapped >= 12), (name, gapped)


def test_params_refuses_an_unknown_field(oracle):
    with pytest.raises(TypeError):
        oracle.params(["-n", "2"], max_bset=3)
    p = oracle.params(["-n", "2"], max_best=7, no_indel_length=-2)
    assert (p.max_diff, p.max_best, p.no_indel_length) == (2, 7, -2)
