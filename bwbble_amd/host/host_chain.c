/*
 * host_chain.c - the host's rules behind the placement records, one function per stage (bwb_host.h): what `aln2sam` and `places2sam` run in
 * whole and `map` runs stage by stage where the GPU cannot (an .ann that is not ascending and disjoint).  A new flag of the result stream
 * gains its host stage here, once.
 */
#include <stdlib.h>
#include <string.h>
#include "bwb_host.h"

void host_outs_open(host_outs_t *out, const map_opts_t *o) {
	out->pile = o->countsFname || o->genoFname ? pile_open(o->countsFname, o->min_mapq) : NULL; /* -A; -G: the table without a file */
	out->indel = o->indelFname || (o->genoFname && o->bubbleFname) ? indel_open(o->indelFname, o->min_mapq, o->anchor) : NULL; /* -I (main.c: only with -B); -G with -B: the table without a file */
	out->geno = o->genoFname ? geno_open(o->genoFname, o->geno_err, o->geno_depth) : NULL; /* -G */
	if (out->pile) { out->pile->min_baseq = o->min_baseq; out->pile->err_cap = o->weighted ? o->geno_err : 0; } /* -b; -Y: the quality sums beside the counters */
	if (out->geno) out->geno->weighted = o->weighted; /* -Y (main.c: only with -G) */
}
void host_outs_free(host_outs_t *out) { pile_free(out->pile); indel_free(out->indel); geno_free(out->geno); }

md_text_t *host_text_open(const char *fastaFname, const map_opts_t *o, const host_outs_t *out, int deferred) {
	return o->md || out->pile ? md_text_open_for(fastaFname, deferred, o->md ? "-D" : o->countsFname ? "-A" : "-G") : NULL;
}

/* (refused tables stop the run before the SAM file exists) */
void host_tables_load(host_tables_t *T, const fasta_annotations_t *ann, const map_opts_t *o, int indel) {
	T->ann = ann; T->ann_sorted = sam_ann_sorted(ann);
	T->bub = o->bubbleFname ? load_bubbles(o->bubbleFname) : NULL;
	T->bubble_of = T->bub ? ann_bubble_of(ann, T->bub) : NULL;
	if (o->lift) lift_check_table(T->bub); /* -R (main.c: only with -B) */
	T->chrom_of = o->join || o->lift || indel ? bubble_chrom_of(ann, T->bubble_of, T->bub, o->join ? "-J" : o->lift ? "-R" : o->indelFname ? "-I" : "-G") : NULL; /* -J (main.c: only with -B and items), -R */
}
void host_tables_free(host_tables_t *T) { free(T->bubble_of); free(T->chrom_of); free_bubbles(T->bub); }

void host_recs_free(host_recs_t *own) {
	free(own->loci); free(own->joins); lift_free(own->lift); md_free(own->md);
	memset(own, 0, sizeof(*own));
}

bwb_locus *host_loci(const sam_reads_t *rd, size_t n, const host_tables_t *T) {
	bwb_locus *loci = (bwb_locus *)malloc((n ? n : 1) * sizeof(bwb_locus));
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
	for (long r = 0; r < (long)n; r++) locus_resolve(&rd->pl[r], T->ann, T->ann_sorted, T->bubble_of, T->bub, &loci[r]);
	return loci;
}

bwb_join *host_joins(const sam_reads_t *rd, size_t n, const host_tables_t *T, int max_mm, const uint8_t *sub, const bwb_aln *hits, const uint64_t *hit_off) {
	const uint64_t *alt_off = rd->alt_off;
	uint8_t *own_sub = sub ? NULL : (uint8_t *)malloc(alt_off[n] ? alt_off[n] : 1);
	bwb_join *joins = (bwb_join *)malloc((n ? n : 1) * sizeof(bwb_join));
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
	for (long r = 0; r < (long)n; r++) {
		if (own_sub) for (uint64_t q = alt_off[r]; q < alt_off[r + 1]; q++) own_sub[q] = hits[hit_off[r] + rd->alts[q].hit].score > hits[hit_off[r]].score;
		join_resolve(&rd->pl[r], &rd->loci[r], rd->alts + alt_off[r], (sub ? sub : own_sub) + alt_off[r], alt_off[r + 1] - alt_off[r], T->ann, T->ann_sorted, T->bubble_of, T->chrom_of, T->bub, max_mm, &joins[r]);
	}
	free(own_sub);
	return joins;
}

void sam_reads_set_lift(sam_reads_t *rd, const lift_set_t *ls) {
	rd->lift_kind = ls ? ls->kind : NULL; rd->lift_off = ls ? ls->off : NULL; rd->lift_recs = ls ? ls->recs : NULL;
}
void sam_reads_set_md(sam_reads_t *rd, const md_set_t *ms) {
	rd->md = ms ? ms->recs : NULL; rd->md_off = ms ? ms->off : NULL; rd->md_text = ms ? ms->text : NULL;
}

void host_chain(sam_reads_t *rd, size_t n, const host_tables_t *T, const map_opts_t *o, const md_text_t *text, const uint8_t *sub, const bwb_aln *hits, const uint64_t *hit_off, int log, host_recs_t *own) {
	memset(own, 0, sizeof(*own));
	rd->bubbles = T->bub;
	rd->loci = own->loci = T->bub ? host_loci(rd, n, T) : NULL;
	rd->joins = own->joins = o->join ? host_joins(rd, n, T, o->max_mm, sub, hits, hit_off) : NULL;
	own->lift = o->lift ? lift_host(rd->pl, rd->loci, n, rd->alt_off, rd->alts, T->ann, T->ann_sorted, T->bubble_of, T->chrom_of, T->bub) : NULL;
	sam_reads_set_lift(rd, own->lift);
	if (own->lift && log) printf("placements lifted to chromosome coordinates on the host: %llu  not liftable %llu\n", (unsigned long long)own->lift->n_lifted, (unsigned long long)own->lift->n_unliftable);
	own->md = o->md ? md_host(rd->pl, n, rd->seq, rd->stride, rd->len, rd->lift_kind, rd->lift_off, rd->lift_recs, T->ann, text) : NULL;
	sam_reads_set_md(rd, own->md);
	if (own->md && log) printf("NM and MD against the text on the host: reads %llu  too long %llu  MD bytes %llu\n", (unsigned long long)own->md->n_ok, (unsigned long long)own->md->n_too_long, (unsigned long long)own->md->off[n]);
}

void host_tail(host_outs_t *out, const sam_reads_t *rd, size_t n, const host_tables_t *T, const md_text_t *text) {
	pile_t *pile = out->pile;
	indel_t *indel = out->indel;
	geno_t *geno = out->geno;
	if (pile) { /* -A: the host's rule on the same records */
		pile_set_text(pile, text, 1);
		pile_host_q(pile, rd->pl, n, rd->seq, rd->stride, rd->len, rd->text, rd->qual_off, rd->lift_kind, rd->lift_off, rd->lift_recs, rd->joins, T->ann);
		if (pile->min_baseq || pile->err_cap) printf("base qualities in the counts on the host: minimum %d  bases dropped %llu  quality sums %s\n", pile->min_baseq, (unsigned long long)pile->dropped, pile->err_cap ? "kept (-Y)" : "not kept");
	}
	if (pile && pile->f) {
		const unsigned long long lines = pile_write(pile, T->ann);
		printf("allele counts at the text's IUPAC sites on the host: sites %llu  reads counted %llu  adds %llu  sites written %llu\n", (unsigned long long)pile->n_sites, (unsigned long long)pile->reads, (unsigned long long)pile->adds, lines);
	}
	if (indel) { /* -I: the host's rule on the same records (the printed CIGAR, with or without -R) */
		indel_set_table(indel, T->bub, T->chrom_of);
		indel_host(indel, rd->pl, rd->loci, n, rd->len, rd->joins);
	}
	if (indel && indel->f) {
		const unsigned long long lines = indel_write(indel);
		printf("read support per indel bubble on the host: anchor %d  eligible bubbles %llu  refused and skipped %llu  reads counted %llu  adds %llu  candidates %llu  lines written %llu\n", indel->anchor,
		       (unsigned long long)indel->n_tab, (unsigned long long)indel->n_refused, (unsigned long long)indel->reads, (unsigned long long)indel->adds, (unsigned long long)indel->cands, lines);
	}
	if (geno) { /* -G: the calls from the two tables, written last */
		geno_host(geno, pile, indel);
		const unsigned long long sites = geno->n_sites, bubs = geno->n_bubs, lines = geno_write(geno, T->ann, T->bub);
		printf("genotype calls on the host: error phred %d  minimum depth %lld  sites called %llu  bubbles called %llu  lines written %llu\n", geno->err, (long long)geno->min_depth, sites, bubs, lines);
	}
}
