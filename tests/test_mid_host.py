"""The five features of `map` together at the next size up, without a GPU: the mid-size fixture of tests/mid_model.py - 3 302 441 characters of
text on 5 chromosomes with 1 200 insertion bubbles, 9 600 searched reads - through the CPU-only chain (the oracle's hits, the models' records,
`places2sam -B t -J [-R [-D -A a -a 1 -I i -w 5]]`).  What the input covers is asserted first; then the chain's bytes against the Python models of
-R, -D, -A and -I, and the placements against the positions the `bwb_synth` reads carry in their names.  tests/test_gpu_mid_stream.py holds
`bwbble map` to the same bytes."""
import re

import pytest

import md_model
import mid_model
import pad_model


@pytest.fixture(scope="module")
def mid(built, oracle, tmp_path_factory):
    return mid_model.build(tmp_path_factory.mktemp("mid_host"), oracle)


def body(sam):
    return [ln.split(b"\t") for ln in sam.split(b"\n")[:-1] if ln[:1] != b"@"]


def test_what_the_input_covers(mid):
    """conditions on the input: enough lifted placements, XA lists, reads at MAPQ 0, sites with a count and adds in every column of the -I table;
    both strands, all five chromosomes; the reads cut across an allele are lifted with an I"""
    j = mid_model.judged(mid)
    lines = body(mid.full)
    assert len(lines) == mid.n_reads == 9600 and len(mid.gen) == 3600 and len(mid.text) == 3_302_441 and len(mid.bubbles) == 1200
    mapped = [f for f in lines if f[1] != b"4"]
    with_bo = [f for f in mapped if f[-1].startswith(b"bO:Z:") or any(t.startswith(b"bO:Z:") for t in f[11:])]
    with_xa = [f for f in mapped if any(t.startswith(b"XA:Z:") for t in f[11:])]
    sites = mid.a_tsv.count(b"\n") - 1
    columns = [int(v) for v in j.counts.sum(axis=0)]
    alt_lifted = sum(1 for f in with_bo if f[0].startswith(b"alt") and b"I" in f[5])
    print(f"lifted {j.n_lifted}  lines with bO {len(with_bo)}  lines with XA {len(with_xa)}  mapped at MAPQ 0 {sum(f[4] == b'0' for f in mapped)}  sites with a count {sites}  "
          f"-I columns {columns}  alt reads lifted with an I {alt_lifted}  unmapped {len(lines) - len(mapped)}  eligible bubbles {j.eligible}")
    assert all(c >= 500 for c in columns), columns
    assert j.n_lifted >= 2000 and len(with_xa) >= 150 and sites >= 5000
    assert {f[1] for f in mapped} == {b"0", b"16"}
    assert {f[2].split()[0] for f in mapped} == {b"chr%d" % c for c in range(1, 6)}
    assert sum(name.startswith("alt") for name, _ in mid.gen) == 1600 and alt_lifted >= 1500


def test_lift_model_writes_the_lifted_bytes(mid):
    j = mid_model.judged(mid)
    assert j.lifted == mid.lifted, pad_model.first_difference(mid.lifted, j.lifted)
    assert j.unliftable == 0 and j.n_lifted >= 2000


def test_md_model_writes_the_full_bytes_and_the_judge_accepts_them(mid):
    j = mid_model.judged(mid)
    assert j.tagged == mid.full, pad_model.first_difference(mid.full, j.tagged)
    bad, n = md_model.judge_sam(mid.full, mid.text, mid.names, mid.starts)
    assert not bad and n == j.census[md_model.OK] > 9000, bad[:3]
    assert j.census[md_model.NONE] == j.census[md_model.TOO_LONG] == 0


def test_pile_model_writes_the_counts(mid):
    j = mid_model.judged(mid)
    assert j.a_tsv == mid.a_tsv, pad_model.first_difference(mid.a_tsv, j.a_tsv)
    assert f"reads counted {j.pile_reads}  adds {j.pile_adds} " in mid.logs["full"]


def test_indel_model_writes_the_table(mid):
    j = mid_model.judged(mid)
    assert j.i_tsv == mid.i_tsv, pad_model.first_difference(mid.i_tsv, j.i_tsv)
    assert f"anchor 5  eligible bubbles {j.eligible}  refused and skipped 0  reads counted {j.indel_reads}  adds {j.indel_adds} " in mid.logs["full"]
    assert j.indel_adds == int(j.counts.sum())


def test_reads_lie_where_their_names_say(mid):
    """every `bwb_synth` read (r<k>_chr<c>_<pos>_<strand>) mapped with MAPQ >= 20 lies on chr<c> within 6 of <pos>: no exception"""
    judged = exceptions = 0
    for f in body(mid.full):
        m = re.fullmatch(rb"r\d+_(chr\d+)_(\d+)_[+-]", f[0])
        if m and f[1] != b"4" and int(f[4]) >= 20:
            judged += 1
            ok = f[2].split()[0] == m.group(1) and abs(int(f[3]) - int(m.group(2))) <= 6
            exceptions += not ok
            if not ok:
                print("exception:", f[:6])
    print(f"{judged} reads judged by their names, {exceptions} exceptions")
    assert judged > 5000 and exceptions == 0
