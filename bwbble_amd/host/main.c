/* main.c - `bwbble` command line, same commands and flags as the reference (mg-aligner/main.c:38-160),
 * plus -g <n_gpus> on align / aln2sam, `map` = align + aln2sam in one pass, and `sampad` = mg-ref/sam_pad (-B on map / aln2sam: the same
 * tags without a second pass; -J, -R, -D, -A, -I and -G, the project's own: placements counted by locus, written in chromosome coordinates, the tags
 * NM:i / MD:Z against the text, the allele counts at the text's IUPAC sites, the read support per indel bubble, and the genotype calls from both;
 * -b and -Y: the base qualities in the counts and the calls). */
#define _GNU_SOURCE
#include <getopt.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>
#include "bwb_host.h"

static int usage(void) {
	printf("Usage:   bwbble command [options] \n");
	printf("Command: index    index sequences in the FASTA format\n");
	printf("         align    exact or inexact read alignment (MI355X)\n");
	printf("         map      align + aln2sam in one pass: FASTQ to SAM (MI355X)\n");
	printf("         fasta2ref    constructs a single linear reference from the input file \n");
	printf("         aln2sam  convert alignment results to SAM file format for single-end mapping\n");
	printf("         sampad   add the reference coordinates of bubble hits to a SAM file (tags bC:Z: / bP:Z:, the reference's sam_pad)\n\n");
	return 1;
}
static int align_usage(void) {
	printf("Usage: bwbble align [options] <seq_fasta> <reads_fastq> <output_aln> \n");
	printf("Options: M    mismatch penalty (default: 3)\n         O    gap open penalty (default: 11) \n         E    gap extend penalty (default: 4) \n");
	printf("         n    maximum number of differences in the alignment (gaps and mismatches) (default: 0)\n");
	printf("         l    length of the seed (seed := first seed_length chars of the read) (default: 32)\n");
	printf("         k    maximum number of differences in the seed (default: 2)\n         o    maximum number of gap opens (default: 1)\n");
	printf("         e    maximum number of gap extends (default: 6) \n         t    accepted for compatibility, ignored (the GPU path has no host threads knob)\n");
	printf("         g    number of GPUs to use (default: 1; more than are present is an error)\n");
	printf("         S    align with a single-genome reference\n         P    use pre-calculated partial alignment results (the GPU computes them per read; <fasta>.pre is written like the reference does when it is missing, and only checked for completeness when present)\n\n");
	return 1;
}

static int map_usage(void) {
	printf("Usage: bwbble map [align options] [-Q <int>] [-X <int>] [-B <bubble.data>] [-J] [-R] [-D] [-A <counts.tsv> [-a <int>]] [-I <indels.tsv> [-w <int>]] [-G <calls.tsv> [-q <int>] [-d <int>]] [-b <int>] [-Y] [-g <gpus>] <seq_fasta> <reads_fastq> <out_sam> \n");
	printf("         writes the SAM file that `bwbble align [align options]` followed by `bwbble aln2sam [-n <Q>] [-X <N>]` writes, without the .aln file\n");
	printf("Options: the options of align, and\n");
	printf("         Q    the mismatch count at which a unique hit gets MAPQ 25 (aln2sam's -n; default: 6)\n");
	printf("         X    1..255: mapped reads get the tags X0:i / X1:i, and a read with 2..X+1 placements lists the others as XA:Z:name,<+|->pos,CIGAR,NM; (default: no tags)\n");
	printf("         B    the bubble table of the multi-genome (bubble.data): reads on a bubble record get the tags bC:Z:<chromosome> bP:Z:<position | lo-hi>, what `bwbble sampad` adds to the SAM file; resolved on the GPU (default: no tags)\n");
	printf("         J    with -X and -B: the placements among a read's XA items that lie where its primary lies - the same chromosome, strand and position, one of them in a bubble record's flank - count as one; MAPQ is computed without them and the read gains bJ:i:<their number> (default: every placement counts)\n");
	printf("         R    with -B: a placement on a bubble record - the read's line and, with -X, every XA item - is written in the chromosome's coordinates: RNAME, POS and a CIGAR with the alternate allele as I and the positions the record skips as D; the line gains bO:Z:<bubble record>,<POS>,<CIGAR> as it was placed; a placement inside the allele alone stays as it is (default: bubble coordinates)\n");
	printf("         D    mapped reads get the tags NM:i:<n> MD:Z:<text> directly behind QUAL, computed on the GPU against the text of <seq_fasta>.ref (`bwbble fasta2ref <seq_fasta>` writes it): a read base that is a member of the text's IUPAC code is a match, a mismatch or deleted position prints the text's letter; with -R a lifted line is described by its chromosome CIGAR; XA items keep their NM (default: no tags)\n");
	printf("         A    writes the allele counts at the IUPAC sites of the text of <seq_fasta>.ref, summed on the GPU over every mapped read: a line `record<TAB>pos<TAB>code<TAB>A<TAB>C<TAB>G<TAB>T` per site that a read base covers under an M of its CIGAR; with -R reads on bubble records count on the chromosome, with -J the joined MAPQ is the one -a sees; the SAM file is the one written without -A (default: no counts)\n");
	printf("         I    with -B: writes the read support per indel bubble, summed on the GPU over every mapped read: a line `bubble<TAB>chrom<TAB>pos<TAB>ref_len<TAB>alt_len<TAB>ref<TAB>alt<TAB>ref_gapped<TAB>alt_gapped` per bubble with a count - reads on the bubble's record that cover the alternate allele and w bases of either flank with M count as alt, reads on the chromosome that cover the site the same way as ref, with an I or D inside as gapped; with -J the joined MAPQ is the one -a sees; the SAM file is the one written without -I (default: no table)\n");
	printf("         G    writes the genotype calls, made on the GPU from the counters of -A and - with -B - of -I, whether or not those files are asked for: after the line `#kind<TAB>record<TAB>pos<TAB>id<TAB>alleles<TAB>AD<TAB>other<TAB>GT<TAB>GQ<TAB>PL` one line S per IUPAC site and one line I per eligible indel bubble with a depth of at least d - the alleles (a site's code members, a bubble's R,V), their read counts, the other bases or gapped reads, the genotype, its quality 0..99 and the phred-scaled likelihoods in VCF order; the SAM, -A and -I files are those written without -G (default: no calls)\n");
	printf("         q    with -G: the error phred, the cost of a base a genotype does not carry, 4..93 (default: 20)\n");
	printf("         d    with -G: the minimum depth of a call, 1..2147483647 (default: 1)\n");
	printf("         w    with -I or -G: the anchor, the flank bases a read must cover on either side, 1..255 (default: 1)\n");
	printf("         a    with -A, -I or -G: only reads with MAPQ >= a count, 0..255 (default: 0)\n");
	printf("         b    with -A or -G: only read bases with a quality of at least b count at a site, 0..93, from the QUAL byte SAM prints under the base; the numbers of -A and the calls of -G are those of the filtered counts; -I is not affected, its rule looks at the CIGAR's ops, not at bases (default: 0)\n");
	printf("         Y    with -G: the calls at the IUPAC sites weigh every counted base by its quality q = min(max(Q, 4), E), E being -q: a genotype pays q for a base it does not carry instead of E; the calls file gains a last column QS, the alleles' quality sums on S lines and `.` on I lines - bubbles are called as without -Y, from -I's counters (default: every base costs E)\n\n");
	return 1;
}
static int aln2sam_usage(void) {
	printf("Usage: bwbble aln2sam [-S, -n, -g, -X, -B, -J, -R, -D, -A, -a, -I, -w, -G, -q, -d, -b, -Y] <seq_fasta> <reads_fastq> <alns_aln> <out_sam> \n");
	printf("Options: n    the mismatch count at which a unique hit gets MAPQ 25 (default: 6)\n         g    number of GPUs for the SA lookups (default: 1)\n");
	printf("         X    1..255: the tags X0:i / X1:i / XA:Z: of `bwbble map -X` (default: no tags)\n");
	printf("         B    the bubble table (bubble.data): the tags bC:Z: / bP:Z: of `bwbble map -B` (default: no tags)\n");
	printf("         J    with -X and -B: MAPQ and the tag bJ:i: of `bwbble map -J` (default: every placement counts)\n");
	printf("         R    with -B: RNAME, POS and CIGAR in chromosome coordinates and the tag bO:Z: of `bwbble map -R` (default: bubble coordinates)\n");
	printf("         D    the tags NM:i: / MD:Z: of `bwbble map -D`, against the text of <seq_fasta>.ref (default: no tags)\n");
	printf("         A    <counts.tsv>: the allele counts of `bwbble map -A`, from the host's rule (default: no counts)\n         I    <indels.tsv>, with -B: the read support per indel bubble of `bwbble map -I`, from the host's rule (default: no table)\n         G    <calls.tsv>: the genotype calls of `bwbble map -G`, from the host's rule (default: no calls)\n         q    with -G: the error phred, 4..93 (default: 20)\n         d    with -G: the minimum depth, 1..2147483647 (default: 1)\n         w    with -I or -G: the anchor, 1..255 (default: 1)\n         a    with -A, -I or -G: the least MAPQ that counts, 0..255 (default: 0)\n         b    with -A or -G: the least base quality that counts at a site, 0..93; -I is not affected (default: 0)\n         Y    with -G: the calls of `bwbble map -Y`, weighted by the base qualities, and the column QS (default: every base costs -q)\n\n");
	return 1;
}
/* a number option's argument: lo..hi, anything else is refused with the flag's own message */
static long long range_option(const char *arg, long long lo, long long hi, const char *refusal) {
	char *end;
	const long long v = strtoll(arg, &end, 10);
	if (end == arg || *end || v < lo || v > hi) { printf(refusal, arg); exit(1); }
	return v;
}

/* the options of the result stream that `map`, `aln2sam` and `places2sam` share (bwb_host.h: map_opts_t): the record before any is given, and
 * one option letter with its argument into it; 0 = not one of them */
static const map_opts_t MAP_OPTS_NONE = { .max_mm = 6 /* (aln2sam's default, mg-aligner/main.c:142) */, .min_mapq = -1 /* (no -a) */, .min_baseq = -1 /* (no -b) */ };
static int map_option(int c, const char *arg, map_opts_t *o) {
	switch (c) {
	case 'Q': o->max_mm = atoi(arg); return 1; /* (aln2sam spells it -n) */
	case 'X': o->max_alt = (int)range_option(arg, 1, 255, "Error: -X takes a number from 1 to 255 (got '%s')\n"); return 1;
	case 'B': o->bubbleFname = arg; return 1;
	case 'J': o->join = 1; return 1;
	case 'R': o->lift = 1; return 1;
	case 'D': o->md = 1; return 1;
	case 'A': o->countsFname = arg; return 1;
	case 'a': o->min_mapq = (int)range_option(arg, 0, 255, "Error: -a takes a MAPQ of 0..255, not %s\n"); return 1;
	case 'I': o->indelFname = arg; return 1;
	case 'w': o->anchor = (int)range_option(arg, 1, 255, "Error: -w takes an anchor of 1..255, not %s\n"); return 1;
	case 'G': o->genoFname = arg; return 1;
	case 'q': o->geno_err = (int)range_option(arg, 4, 93, "Error: -q takes an error phred of 4..93, not %s\n"); return 1;
	case 'b': o->min_baseq = (int)range_option(arg, 0, 93, "Error: -b takes a base quality of 0..93, not %s\n"); return 1;
	case 'Y': o->weighted = 1; return 1;
	case 'd': o->geno_depth = range_option(arg, 1, 2147483647ll, "Error: -d takes a minimum depth of 1..2147483647, not %s\n"); return 1;
	}
	return 0;
}

/* what one flag needs of another, in this order: -J, -R, -a, -I / -w, -q / -d, -b, -Y; then the defaults of what was not given */
static void map_opts_finish(map_opts_t *o) {
	const char *B = o->bubbleFname;
	if (o->join && !(o->max_alt && B)) { printf("Error: -J needs %s%s%s\n", o->max_alt ? "" : "-X <N>", o->max_alt || B ? "" : " and ", B ? "" : "-B <bubble.data>"); exit(1); }
	if (o->lift && !B) { printf("Error: -R needs -B <bubble.data>\n"); exit(1); }
	if (o->min_mapq >= 0 && !o->countsFname && !o->indelFname && !o->genoFname) { printf("Error: -a needs -A <counts.tsv>, -I <indels.tsv> or -G <calls.tsv>\n"); exit(1); }
	if (o->indelFname && !B) { printf("Error: -I needs -B <bubble.data>\n"); exit(1); }
	if (o->anchor && !o->indelFname && !o->genoFname) { printf("Error: -w needs -I <indels.tsv> or -G <calls.tsv>\n"); exit(1); }
	if (o->geno_err && !o->genoFname) { printf("Error: -q needs -G <calls.tsv>\n"); exit(1); }
	if (o->geno_depth && !o->genoFname) { printf("Error: -d needs -G <calls.tsv>\n"); exit(1); }
	if (o->min_baseq >= 0 && !o->countsFname && !o->genoFname) { printf("Error: -b needs -A <counts.tsv> or -G <calls.tsv>\n"); exit(1); }
	if (o->weighted && !o->genoFname) { printf("Error: -Y needs -G <calls.tsv>\n"); exit(1); }
	if (o->min_mapq < 0) o->min_mapq = 0;
	if (o->min_baseq < 0) o->min_baseq = 0;
	if (!o->anchor) o->anchor = 1;
	if (!o->geno_err) o->geno_err = 20;
	if (!o->geno_depth) o->geno_depth = 1;
}

/* the options `align` and `map` share; 0 = not one of them */
static int align_option(int c, aln_params_t *params, int *n_gpus) {
	switch (c) {
	case 'M': params->mm_score = atoi(optarg); return 1;
	case 'O': params->gapo_score = atoi(optarg); return 1;
	case 'E': params->gape_score = atoi(optarg); return 1;
	case 'n': params->max_diff = atoi(optarg); return 1;
	case 'k': params->max_diff_seed = atoi(optarg); return 1;
	case 'o': params->max_gapo = atoi(optarg); return 1;
	case 'e': params->max_gape = atoi(optarg); return 1;
	case 'l': params->seed_length = atoi(optarg); return 1;
	case 'm': params->max_entries = atoi(optarg); return 1;
	case 't': params->n_threads = atoi(optarg); return 1;
	case 'g': *n_gpus = atoi(optarg); return 1;
	case 'S': params->is_multiref = 0; return 1;
	case 'P': params->use_precalc = 1; return 1;
	}
	return 0;
}

int main(int argc, char *argv[]) {
	if (argc < 2) return usage();
	if (strcmp(argv[1], "index") == 0) {
		if (argc < 3) { printf("Usage: bwbble index [options] <seq_fasta> \n"); exit(1); }
		char *esa = NULL;
		int c;
		while ((c = getopt(argc - 1, argv + 1, "e:")) >= 0) {
			if (c == 'e') esa = optarg; else return 1;
		}
		index_bwt(argv[optind + 1], esa);
	} else if (strcmp(argv[1], "align") == 0) {
		if (argc < 5) { align_usage(); exit(1); }
		aln_params_t params;
		set_default_aln_params(&params);
		int c, n_gpus = 1;
		while ((c = getopt(argc - 1, argv + 1, "M:O:E:n:k:o:e:l:m:t:g:SP")) >= 0) {
			if (align_option(c, &params, &n_gpus)) continue;
			if (c == '?') { align_usage(); return 1; }
			return 1;
		}
		if (argc - 1 - optind < 3) { align_usage(); exit(1); }
		align_reads(argv[optind + 1], argv[optind + 2], argv[optind + 3], &params, n_gpus);
	} else if (strcmp(argv[1], "map") == 0) {
		if (argc < 5) { map_usage(); exit(1); }
		aln_params_t params;
		set_default_aln_params(&params);
		int c, n_gpus = 1;
		map_opts_t o = MAP_OPTS_NONE;
		while ((c = getopt(argc - 1, argv + 1, "M:O:E:n:k:o:e:l:m:t:g:SPQ:X:B:JRDA:a:I:w:G:q:d:b:Y")) >= 0) {
			if (align_option(c, &params, &n_gpus) || map_option(c, optarg, &o)) continue;
			if (c == '?') { map_usage(); return 1; }
			return 1;
		}
		if (argc - 1 - optind < 3) { map_usage(); exit(1); }
		map_opts_finish(&o);
		map_reads(argv[optind + 1], argv[optind + 2], argv[optind + 3], &params, &o, n_gpus);
	} else if (strcmp(argv[1], "places2sam") == 0) {
		/* developer command (CPU only, used by the tests): placement records (bwb_place, include/bwbble_hip.h) from a file -> SAM text */
		/* (a sixth argument: u64 alt_off[n + 1] followed by the bwb_alt records - the X tags of `map -X`) */
		/* (a leading `-B <bubble.data>`: the tags of `map -B`, the loci from the host resolver; `-J` behind it: MAPQ and the tag of `map -J`,
		 * the items file then ends with one byte per item, not zero for a suboptimal one; `-R` behind them: RNAME, POS and CIGAR of `map -R`, from the
		 * host's rule; `-D` behind that: the tags NM / MD of `map -D`, from the host's rule; `-A <counts.tsv>` and `-a <MAPQ>` behind that: the allele
		 * counts of `map -A`, from the host's rule; `-I`, `-w`, `-G`, `-q`, `-d` and last `-b <m>` and `-Y`: the tables and calls of the flags of `map`) */
		/* (the flags only in this order, each at most once) */
		char **a = argv + 2;
		int na = argc - 2;
		map_opts_t o = MAP_OPTS_NONE;
		for (const char *f = "B:JRDA:a:I:w:G:q:d:b:Y"; *f; f++) {
			const int arg = f[1] == ':';
			if (na > arg && a[0][0] == '-' && a[0][1] == *f && !a[0][2]) { map_option(*f, arg ? a[1] : NULL, &o); a += 1 + arg; na -= 1 + arg; }
			f += arg;
		}
		if (na < 4) { printf("Usage: bwbble places2sam [-B <bubble.data>] [-J] [-R] [-D] [-A <counts.tsv>] [-a <MAPQ>] [-I <indels.tsv>] [-w <anchor>] [-G <calls.tsv>] [-q <err>] [-d <depth>] [-b <baseq>] [-Y] <seq_fasta> <reads_fastq> <places_bin> <out_sam> [<alts_bin>] \n"); exit(1); }
		o.max_alt = na >= 5; /* (-J needs the items file, as it needs -X elsewhere) */
		map_opts_finish(&o);
		places2sam(a[0], a[1], a[2], a[3], na >= 5 ? a[4] : NULL, &o);
	} else if (strcmp(argv[1], "sampad") == 0) {
		if (argc < 5) { printf("Usage: bwbble sampad <bubble.data> <in_sam> <out_sam> \n"); exit(1); }
		sam_pad(argv[2], argv[3], argv[4]);
	} else if (strcmp(argv[1], "fasta2ref") == 0) {
		if (argc < 3) { printf("Usage: bwbble fasta2ref <seq_fasta> \n"); exit(1); }
		size_t L = strlen(argv[2]) + 8;
		char *refFname = (char *)malloc(L), *annFname = (char *)malloc(L);
		snprintf(refFname, L, "%s.ref", argv[2]);
		snprintf(annFname, L, "%s.ann", argv[2]);
		unsigned char *seq;
		bwtint_t seqLen;
		fasta2ref(argv[2], refFname, annFname, &seq, &seqLen);
		free(seq); free(refFname); free(annFname);
	} else if (strcmp(argv[1], "aln2sam") == 0) {
		if (argc < 6) { aln2sam_usage(); exit(1); }
		int is_multiref = 1, n_gpus = 1, c;
		map_opts_t o = MAP_OPTS_NONE;
		while ((c = getopt(argc - 1, argv + 1, "n:g:SX:B:JRDA:a:I:w:G:q:d:b:Y")) >= 0) {
			if (map_option(c == 'n' ? 'Q' : c, optarg, &o)) continue;
			switch (c) {
			case 'S': is_multiref = 0; break;
			case 'g': n_gpus = atoi(optarg); break;
			case '?': printf("Unknown option \n"); break;
			default: return 1;
			}
		}
		if (argc - 1 - optind < 4) { aln2sam_usage(); exit(1); }
		map_opts_finish(&o);
		alns2sam(argv[optind + 1], argv[optind + 2], argv[optind + 3], argv[optind + 4], is_multiref, n_gpus, &o);
	} else if (strcmp(argv[1], "dumpreads") == 0) {
		/* developer command (CPU only, used by the tests): what fastq2reads made of a FASTQ - per read "name<TAB>codes<TAB>quality" */
		if (argc < 4) { printf("Usage: bwbble dumpreads <reads_fastq> <out_tsv> [chunk_reads [text]] \n"); exit(1); }
		if (argc >= 5) { /* the streaming reader of `align` (fq_next_chunk), chunk by chunk: "codes" per read */
			/* (a sixth argument `text`: the stream of `map`, fq_open_text - "name<TAB>codes<TAB>quality" like the whole-file form) */
			const int text = argc >= 6 && strcmp(argv[5], "text") == 0;
			fq_stream *fs = text ? fq_open_text(argv[2]) : fq_open(argv[2]);
			FILE *g = fopen(argv[3], "w");
			if (!g) { perror(argv[3]); return 1; }
			fq_chunk_t ch;
			while (fq_next_chunk(fs, (uint32_t)atoi(argv[4]), &ch)) {
				for (uint32_t r = 0; r < ch.n; r++) {
					if (text) {
						fprintf(g, "%.*s\t", (int)ch.name_len[r], ch.text + ch.name_off[r]);
						for (uint32_t i = 0; i < ch.len[r]; i++) fputc('0' + ch.seq[(size_t)r * ch.stride + i], g);
						fprintf(g, "\t%.*s\n", (int)ch.len[r], ch.text + ch.qual_off[r]);
						continue;
					}
					for (uint32_t i = 0; i < ch.stride; i++) if (i < ch.len[r]) fputc('0' + ch.seq[(size_t)r * ch.stride + i], g); else if (ch.seq[(size_t)r * ch.stride + i] != 4) fputc('!', g);
					fputc('\n', g);
				}
				free(ch.seq); free(ch.len); free(ch.name_off); free(ch.qual_off); free(ch.name_len);
			}
			fclose(g);
			fq_close(fs);
			return 0;
		}
		reads_t *reads = fastq2reads(argv[2]);
		FILE *f = fopen(argv[3], "w");
		if (!f) { perror(argv[3]); return 1; }
		for (unsigned r = 0; r < reads->count; r++) {
			fprintf(f, "%.*s\t", (int)reads->name_len[r], reads->raw + reads->name_off[r]);
			for (int i = 0; i < reads->len[r]; i++) fputc('0' + reads->seq[(size_t)r * reads->stride + i], f);
			fprintf(f, "\t%.*s\n", (int)reads->len[r], reads->raw + reads->qual_off[r]);
		}
		fclose(f);
		free_reads(reads);
	} else if (strcmp(argv[1], "bwtcat") == 0) {
		/* developer command (CPU only, used by the tests): .bwt -> memory through the threaded loader (load_bwt_start / blocks_ready) -> .bwt */
		if (argc < 4) { printf("Usage: bwbble bwtcat <in_bwt> <out_bwt> \n"); exit(1); }
		bwt_t *B = load_bwt_start(argv[2], 1);
		uint64_t last = 0;
		while (B->loader && last < B->num_occ) { const uint64_t r = __atomic_load_n(&B->blocks_ready, __ATOMIC_ACQUIRE); if (r < last) { printf("blocks_ready went backwards\n"); return 1; } last = r; if (r >= B->num_occ) break; }
		load_bwt_wait(B);
		if (B->blocks_ready != B->num_occ) { printf("blocks_ready %llu != %llu\n", (unsigned long long)B->blocks_ready, (unsigned long long)B->num_occ); return 1; }
		store_bwt(B, argv[3]);
		free_bwt(B);
	} else if (strcmp(argv[1], "alncat") == 0) {
		/* developer command (CPU only, used by the tests): .aln -> memory (alnsf2alns_bin) -> .aln (alns2alnf_bin read by read, or with a
		 * fifth argument `buf` the chunk serialiser of `align`, alns2alnf_buf, in chunks of a few reads) */
		if (argc < 4) { printf("Usage: bwbble alncat <in_aln> <out_aln> [buf [chunk_reads]]\n"); exit(1); }
		alns_batch_t *b = alnsf2alns_bin(argv[2]);
		FILE *f = fopen(argv[3], "wb");
		if (!f) { perror(argv[3]); return 1; }
		if (argc >= 5) {
			const size_t chunk = argc >= 6 ? (size_t)atol(argv[5]) : 1000;
			for (size_t r0 = 0; r0 < b->n_reads; r0 += chunk) {
				const size_t n = b->n_reads - r0 < chunk ? b->n_reads - r0 : chunk;
				uint64_t *off = (uint64_t *)malloc((n + 1) * 8); /* (chunk-relative, like a slot's result) */
				for (size_t k = 0; k <= n; k++) off[k] = b->aln_off[r0 + k] - b->aln_off[r0];
				size_t len = 0;
				unsigned char *buf = alns2alnf_buf(b->alns + b->aln_off[r0], off, (uint32_t)n, &len);
				fwrite(buf, 1, len, f);
				free(buf); free(off);
			}
		} else for (size_t r = 0; r < b->n_reads; r++) alns2alnf_bin(b->alns + b->aln_off[r], b->aln_off[r + 1] - b->aln_off[r], f);
		fclose(f);
		free_alns_batch(b);
	} else if (strcmp(argv[1], "hostbench") == 0) {
		/* developer command (CPU only; bench.py's host_pipeline keys): the two host stages of `align` on their own - the FASTQ reader
		 * (parallel record scan + base encoding, reads.c) in chunks of BWB_CHUNK reads, and the chunk serialiser (aln_io.c) on an .aln file */
		if (argc < 3) { printf("Usage: bwbble hostbench <reads_fastq> [<aln>]\n"); exit(1); }
		struct timespec t0, t1;
		const uint32_t chunk = getenv("BWB_CHUNK") ? (uint32_t)strtoul(getenv("BWB_CHUNK"), NULL, 10) : GPU_CHUNK_DEFAULT;
		clock_gettime(CLOCK_MONOTONIC, &t0);
		fq_stream *fs = fq_open(argv[2]);
		fq_chunk_t ch;
		uint64_t n = 0, cks = 0;
		while (fq_next_chunk(fs, chunk, &ch)) { n += ch.n; cks += ch.seq[(size_t)(ch.n - 1) * ch.stride] + ch.len[0]; free(ch.seq); free(ch.len); }
		fq_close(fs);
		clock_gettime(CLOCK_MONOTONIC, &t1);
		double dt = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
		extern double fq_prof_s[3];
		printf("{\"parse_reads\": %llu, \"parse_s\": %.4f, \"parse_reads_per_s\": %.0f, \"parse_stages_s\": {\"scan\": %.3f, \"alloc\": %.3f, \"encode\": %.3f}, \"checksum\": %llu", (unsigned long long)n, dt, n / (dt > 0 ? dt : 1), fq_prof_s[0], fq_prof_s[1], fq_prof_s[2], (unsigned long long)cks);
		if (argc >= 4) {
			alns_batch_t *b = alnsf2alns_bin(argv[3]);
			double best = 1e30; size_t bytes = 0;
			for (int rep = 0; rep < 3; rep++) {
				clock_gettime(CLOCK_MONOTONIC, &t0);
				bytes = 0;
				for (size_t r0 = 0; r0 < b->n_reads; r0 += chunk) {
					const size_t nn = b->n_reads - r0 < chunk ? b->n_reads - r0 : chunk;
					uint64_t *off = (uint64_t *)malloc((nn + 1) * 8);
					for (size_t k = 0; k <= nn; k++) off[k] = b->aln_off[r0 + k] - b->aln_off[r0];
					size_t len = 0;
					unsigned char *buf = alns2alnf_buf(b->alns + b->aln_off[r0], off, (uint32_t)nn, &len);
					bytes += len;
					free(buf); free(off);
				}
				clock_gettime(CLOCK_MONOTONIC, &t1);
				dt = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
				if (dt < best) best = dt;
			}
			printf(", \"write_records\": %zu, \"write_bytes\": %zu, \"serialise_s\": %.4f, \"write_records_per_s\": %.0f", b->n_reads, bytes, best, b->n_reads / (best > 0 ? best : 1));
			free_alns_batch(b);
		}
		printf("}\n");
	} else {
		printf("Error: Unknown command '%s'\n", argv[1]);
		usage();
	}
	return 0;
}
