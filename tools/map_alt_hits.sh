#!/bin/bash
# What `map -X` costs, and that `map` without -X costs nothing: this tree's `bwbble map` against another build's - the parent commit's -
# back to back on one machine.  chr21-scale index (48 M forward characters), 10 M x 100 bp reads (the input of tools/map_vs_two_pass.sh),
# -n 3 and -n 0: three runs of each build, alternating, then `map -X 5` twice; wall time from process start to exit.  The SAM files
# without -X are compared byte for byte, the -X file's columns 1-11 with them.  Every step has its own time limit; the first failure ends
# the script.
# usage: tools/map_alt_hits.sh <the other build's bwbble_amd/bin> [output directory]     (run from the repository root)
set -u
[ $# -ge 1 ] || { echo "usage: $0 <other build's bwbble_amd/bin> [output directory]"; exit 2; }
OUT=${2:-$PWD/map_alt_hits_out}; mkdir -p $OUT
LOG=$OUT/map_alt_hits_raw.txt; : > $LOG
W=/tmp/bwb_alt_meas_$$; mkdir -p $W
NEW=$PWD/bwbble_amd/bin; OLD=$1
step() { # step <seconds> <label> <command...>: wall time of the command, its output to the log
	local lim=$1 label=$2; shift 2
	cat $W/g.fa.bwt $W/r.fq > /dev/null 2>&1   # same page-cache state for every timed command
	local t0=$(date +%s.%N)
	timeout -k 10 $lim "$@" >> $LOG 2>&1; local rc=$?
	local t1=$(date +%s.%N)
	echo "### $label rc=$rc wall_s=$(awk "BEGIN{printf \"%.2f\", $t1-$t0}")" | tee -a $LOG
	return $rc
}
step 300 synth_genome $NEW/bwb_synth genome $W/g.fa 48000000 1 20000 21 &&
step 900 index $NEW/bwbble index $W/g.fa &&
step 300 synth_reads $NEW/bwb_synth reads $W/g.fa $W/r.fq 10000000 100 1000 1.0 0.1 0.0 || { rm -rf $W; exit 1; }
rm -f $W/g.fa.ref
for n in 3 0; do
	for k in 1 2 3; do
		step 600 "parent_map_n${n}_run$k" $OLD/bwbble map -n $n $W/g.fa $W/r.fq $W/p.sam &&
		step 600 "this_map_n${n}_run$k" $NEW/bwbble map -n $n $W/g.fa $W/r.fq $W/m.sam || { rm -rf $W; exit 1; }
	done
	step 600 "this_map_n${n}_X5_run1" $NEW/bwbble map -n $n -X 5 $W/g.fa $W/r.fq $W/x.sam &&
	step 600 "this_map_n${n}_X5_run2" $NEW/bwbble map -n $n -X 5 $W/g.fa $W/r.fq $W/x.sam || { rm -rf $W; exit 1; }
	if cmp -s $W/p.sam $W/m.sam; then echo "### sam_identical_n$n yes ($(stat -c %s $W/m.sam) bytes without -X, $(stat -c %s $W/x.sam) with -X 5)" | tee -a $LOG; else echo "### sam_identical_n$n NO" | tee -a $LOG; rm -rf $W; exit 1; fi
	if cmp -s <(cut -f 1-11 $W/x.sam) $W/m.sam; then echo "### columns_1_11_identical_n$n yes ($(grep -c "XA:Z:" $W/x.sam) reads list other placements)" | tee -a $LOG; else echo "### columns_1_11_identical_n$n NO" | tee -a $LOG; rm -rf $W; exit 1; fi
	rm -f $W/*.sam
done
rm -rf $W
grep -E "^###|placements on|^GPUs:" $LOG > $OUT/map_alt_hits.txt
python3 - $OUT/map_alt_hits.txt >> $OUT/map_alt_hits.txt <<'PY'
import re, statistics, sys
t = {}
for ln in open(sys.argv[1]):
    m = re.match(r"### (parent|this)_map_n(\d)(_X5)?_run\d rc=0 wall_s=([0-9.]+)", ln)
    if m:
        t.setdefault((m.group(1), m.group(2), bool(m.group(3))), []).append(float(m.group(4)))
print("#")
for n in ("3", "0"):
    p, q, x = t[("parent", n, False)], t[("this", n, False)], t[("this", n, True)]
    spread = max(p) - min(p)
    verdict = "within" if statistics.median(q) - statistics.median(p) <= spread else "OUTSIDE"
    print(f"# -n {n}: parent median {statistics.median(p):.2f} s (min {min(p):.2f}, max {max(p):.2f}, spread {spread:.2f}) | this median {statistics.median(q):.2f} s "
          f"(difference {statistics.median(q) - statistics.median(p):+.2f} s: {verdict} the parent's spread) | -X 5: {min(x):.2f} s, {max(x):.2f} s")
PY
cat $OUT/map_alt_hits.txt
