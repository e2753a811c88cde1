#!/bin/bash
# `bwbble map` of this tree against the two-pass route (align + aln2sam) of another build - the parent commit's -, back to back on one
# machine: chr21-scale index (48 M forward characters), 10 M x 100 bp reads, -n 0 and -n 3; wall time from process start to exit, the
# SAM files compared byte for byte.  Every step has its own time limit; the first failure ends the script.
# usage: tools/map_vs_two_pass.sh <the other build's bwbble_amd/bin> [output directory]     (run from the repository root)
set -u
[ $# -ge 1 ] || { echo "usage: $0 <other build's bwbble_amd/bin> [output directory]"; exit 2; }
OUT=${2:-$PWD/map_vs_two_pass_out}; mkdir -p $OUT
LOG=$OUT/map_vs_two_pass_raw.txt; : > $LOG
W=/tmp/bwb_map_meas_$$; mkdir -p $W
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
for n in 0 3; do
	step 600 "parent_align_n$n" $OLD/bwbble align -n $n $W/g.fa $W/r.fq $W/p$n.aln &&
	step 600 "parent_aln2sam_n$n" $OLD/bwbble aln2sam $W/g.fa $W/r.fq $W/p$n.aln $W/p$n.sam &&
	step 600 "map_n$n" $NEW/bwbble map -n $n $W/g.fa $W/r.fq $W/m$n.sam &&
	step 600 "parent_align_again_n$n" $OLD/bwbble align -n $n $W/g.fa $W/r.fq $W/p$n.b.aln &&
	step 600 "map_again_n$n" $NEW/bwbble map -n $n $W/g.fa $W/r.fq $W/m$n.b.sam || { rm -rf $W; exit 1; }
	if cmp -s $W/p$n.sam $W/m$n.sam && cmp -s $W/m$n.sam $W/m$n.b.sam; then echo "### sam_identical_n$n yes ($(stat -c %s $W/m$n.sam) bytes, aln $(stat -c %s $W/p$n.aln) bytes)" | tee -a $LOG; else echo "### sam_identical_n$n NO" | tee -a $LOG; rm -rf $W; exit 1; fi
	rm -f $W/*.aln $W/*.sam
done
rm -rf $W
grep -E "^###|SA lookups|placements on|start-up:|^GPUs:" $LOG > $OUT/map_vs_two_pass.txt
cat $OUT/map_vs_two_pass.txt
