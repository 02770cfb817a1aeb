/*
 * rphmm_result.c -- what both host paths end in: the genome fragment of a traced-back path and the mrp_phase_result
 * built from it (emissions.c:246-343, genomeFragment.c, bubbleGraph.c:2761-2779), on the flat hmm of rphmm_common.h.
 * The per-chunk path (rphmm_chunk.c) comes here with an hmm it swept itself; the device-resident path (rphmm_host.c)
 * only for a chunk whose fragment the device did not leave, and for the result's arrays.  Host only: nothing here
 * touches the device.
 *
 * Also here, because both paths call them and none is worth a copy per file: the checks of a call's chunk and reads
 * (world_init, world_host), the stable sort both coverage filters use, and the end of a flat hmm and of a result.
 * Everything is allocated from the heap (see the scratch arena in rphmm_host.c).
 */
#define _GNU_SOURCE
#include "rphmm_common.h"

static int check_reads(const world *w, const mrp_read *reads, int64_t n) {
    for (int64_t i = 0; i < n; i++) {
        const mrp_read *r = &reads[i];
        if (!r->name || r->length < 1 || r->ref_start < 0 || (int64_t) r->ref_start + r->length > w->ch.n_sites)
            return mrp_set_error(MRP_ERR_ARG, "read %lld: bad interval [%d,+%d)", (long long) i, r->ref_start, r->length);
        const int64_t nb = w->ch.allele_offset[r->ref_start + r->length] - w->ch.allele_offset[r->ref_start];
        if (r->pool_offset < 0 || r->pool_offset + nb > w->ch.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "read %lld: profile bytes outside the pool", (long long) i);
    }
    return MRP_OK;
}
int world_init(world *w, mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads,
               mrp_batch *record) {
    if (!ctx || !chunk || (n_reads > 0 && !reads)) return mrp_set_error(MRP_ERR_ARG, "NULL argument");
    if (mrp_context_device(mrp_chunk_context(chunk)) != mrp_context_device(ctx)) return mrp_set_error(MRP_ERR_ARG, "chunk lives on a different device");
    memset(w, 0, sizeof(*w));
    w->chunk = chunk; w->reads = reads; w->n_reads = n_reads; w->ctx = ctx; w->record = record;
    mrp_chunk_host_view(chunk, &w->ch);
    w->max_alleles = 1;
    for (int64_t i = 0; i < w->ch.n_sites; i++) if (w->ch.allele_number[i] > w->max_alleles) w->max_alleles = w->ch.allele_number[i];
    return check_reads(w, reads, n_reads);
}
int world_host(world *w, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads) {
    if (!chunk || (n_reads > 0 && !reads)) return mrp_set_error(MRP_ERR_ARG, "NULL argument");
    memset(w, 0, sizeof(*w));
    w->chunk = chunk; w->reads = reads; w->n_reads = n_reads;
    mrp_chunk_host_view(chunk, &w->ch);
    return check_reads(w, reads, n_reads);
}

void keyed_sort_desc(keyed *a, int64_t n, keyed *tmp) { /* stable, descending */
    for (int64_t wdt = 1; wdt < n; wdt *= 2) {
        for (int64_t lo = 0; lo < n; lo += 2 * wdt) {
            const int64_t mid = lo + wdt < n ? lo + wdt : n, hi = lo + 2 * wdt < n ? lo + 2 * wdt : n;
            int64_t i = lo, j = mid, o = lo;
            while (i < mid && j < hi) { if (a[j].key > a[i].key) tmp[o++] = a[j++]; else tmp[o++] = a[i++]; }
            while (i < mid) tmp[o++] = a[i++];
            while (j < hi) tmp[o++] = a[j++];
        }
        memcpy(a, tmp, sizeof(keyed) * (size_t) n);
    }
}

void mrp_hmm_destroy(mrp_hmm *h) {
    if (!h) return;
    void *arrays[] = {h->reads.a, h->col_start.a, h->col_len.a, h->col_depth.a, h->cell_off.a, h->read_off.a, h->col_reads.a,
                      h->read_byte_off.a, h->part.a, h->next.a, h->prev.a, h->mask_from.a, h->mask_to.a, h->mcell_off.a,
                      h->mfrom.a, h->mto.a};
    for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); i++) hmm_free_array(h, arrays[i]);
    hmm_free_results(h);
    free(h);
}
void mrp_free(void *p) { free(p); }

/* ------------------------------------------------------------------------------------------ */
/* genome fragment (emissions.c:246-343, genomeFragment.c)                                     */
/* ------------------------------------------------------------------------------------------ */
mrp_phase_result *result_new(int32_t ref_start, int32_t length, int64_t n_reads) {
    mrp_phase_result *r = xcalloc(1, sizeof(*r));
    r->ref_start = ref_start; r->length = length;
    const size_t n = (size_t) length;
    r->genotype_string = xcalloc(n, sizeof(uint64_t)); r->haplotype_string1 = xcalloc(n, sizeof(uint64_t));
    r->haplotype_string2 = xcalloc(n, sizeof(uint64_t)); r->ancestor_string = xcalloc(n, sizeof(uint64_t));
    r->reads_supporting_haplotype1 = xcalloc(n, sizeof(uint64_t)); r->reads_supporting_haplotype2 = xcalloc(n, sizeof(uint64_t));
    r->genotype_probs = xcalloc(n, sizeof(float)); r->haplotype_probs1 = xcalloc(n, sizeof(float));
    r->haplotype_probs2 = xcalloc(n, sizeof(float));
    /* (a read that inconsistent columns put on both sides sits in both lists and may be moved into a list that already holds it) */
    r->reads1 = xcalloc(2 * (size_t) n_reads + 2, sizeof(int32_t)); r->reads2 = xcalloc(2 * (size_t) n_reads + 2, sizeof(int32_t));
    return r;
}
void mrp_phase_result_destroy(mrp_phase_result *r) {
    if (!r) return;
    free(r->genotype_string); free(r->haplotype_string1); free(r->haplotype_string2); free(r->ancestor_string);
    free(r->reads_supporting_haplotype1); free(r->reads_supporting_haplotype2); free(r->genotype_probs);
    free(r->haplotype_probs1); free(r->haplotype_probs2); free(r->reads1); free(r->reads2);
    free(r);
}
/* fillInPredictedGenome emissions.c:323-343 for column k with the given partition.  The allele
 * costs are the same integers getLogProbOfAllele returns (sum of the bytes of the reads in the
 * partition), summed directly. */
static void fill_in_predicted_genome(const world *w, mrp_phase_result *g, const mrp_hmm *h, int64_t k, uint64_t partition, uint64_t *scratch) {
    const int32_t depth = h->col_depth.a[k];
    const int64_t *off = h->read_byte_off.a + h->read_off.a[k];
    const int32_t start = h->col_start.a[k];
    const uint32_t first_allele = w->ch.allele_offset[start];
    uint64_t *h1 = scratch, *h2 = h1 + w->max_alleles, *a1 = h2 + w->max_alleles, *a2 = a1 + w->max_alleles; /* [4 * max_alleles] */
    for (int32_t s = 0; s < h->col_len.a[k]; s++) {
        const int32_t site = start + s;
        const uint32_t A = w->ch.allele_number[site], so = w->ch.allele_offset[site] - first_allele;
        const uint16_t *sub = w->ch.sub + w->ch.sub_offset[site], *prior = w->ch.prior + w->ch.allele_offset[site];
        if (A == 2) { /* the common case: both bytes of a read together, no branch on the partition bit */
            uint64_t t0 = 0, t1 = 0, x0 = 0, x1 = 0; /* totals over the column's reads, and over those in the partition */
            for (int32_t i = 0; i < depth; i++) {
                const uint8_t *b = w->ch.pool + off[i] + so;
                const uint64_t in = 0 - ((partition >> i) & 1);
                t0 += b[0]; t1 += b[1];
                x0 += b[0] & in; x1 += b[1] & in;
            }
            h1[0] = x0; h1[1] = x1; h2[0] = t0 - x0; h2[1] = t1 - x1;
        } else {
            for (uint32_t a = 0; a < A; a++) { h1[a] = 0; h2[a] = 0; }
            for (int32_t i = 0; i < depth; i++) {
                const uint8_t *b = w->ch.pool + off[i] + so;
                uint64_t *dst = ((partition >> i) & 1) ? h1 : h2;
                for (uint32_t a = 0; a < A; a++) dst[a] += b[a];
            }
        }
        for (uint32_t i = 0; i < A; i++) { /* ancestorHapProbabilities emissions.c:156-172 */
            uint64_t x = h1[0] + sub[i * A], y = h2[0] + sub[i * A];
            for (uint32_t q = 1; q < A; q++) {
                if (h1[q] + sub[i * A + q] < x) x = h1[q] + sub[i * A + q];
                if (h2[q] + sub[i * A + q] < y) y = h2[q] + sub[i * A + q];
            }
            a1[i] = x; a2[i] = y;
        }
        uint64_t best = a1[0] + a2[0] + prior[0], anc = 0; /* :283-292 */
        for (uint32_t i = 1; i < A; i++) {
            const uint64_t j = a1[i] + a2[i] + prior[i];
            if (j < best) { best = j; anc = i; }
        }
        uint64_t hap1 = 0, hap2 = 0, m1 = h1[0] + sub[anc * A], m2 = h2[0] + sub[anc * A]; /* getMLAllele :246-261 */
        for (uint32_t i = 1; i < A; i++) {
            if (h1[i] + sub[anc * A + i] < m1) { m1 = h1[i] + sub[anc * A + i]; hap1 = i; }
            if (h2[i] + sub[anc * A + i] < m2) { m2 = h2[i] + sub[anc * A + i]; hap2 = i; }
        }
        const int64_t q = site - g->ref_start;
        g->ancestor_string[q] = anc;
        g->haplotype_string1[q] = hap1;
        g->haplotype_string2[q] = hap2;
        g->genotype_string[q] = hap1 < hap2 ? hap1 * A + hap2 : hap2 * A + hap1;
        g->genotype_probs[q] = -((float) best);
        g->haplotype_probs1[q] = -(float) h1[hap1];
        g->haplotype_probs2[q] = -(float) h2[hap2];
        g->reads_supporting_haplotype1[q] = (uint64_t) __builtin_popcountll(partition);
        g->reads_supporting_haplotype2[q] = (uint64_t) depth - (uint64_t) __builtin_popcountll(partition);
    }
}
/* getLogProbOfReadGivenHaplotype genomeFragment.c:71-89, for both haplotypes in one walk over the read's sites: *x for hap1,
 * *y for hap2 (each sum in site order, then divided by PROFILE_PROB_SCALAR inc/margin.h:189) */
static void read_log_prob2(const world *w, const uint64_t *hap1, const uint64_t *hap2, int32_t start, int32_t length, int32_t read, double *x, double *y) {
    const mrp_read *r = &w->reads[read];
    double t1 = 0.0, t2 = 0.0;
    const uint32_t first = w->ch.allele_offset[r->ref_start];
    int32_t lo = start - r->ref_start, hi = start + length - r->ref_start;
    if (lo < 0) lo = 0;
    if (hi > r->length) hi = r->length;
    const uint8_t *pool = w->ch.pool + r->pool_offset;
    const uint32_t *ao = w->ch.allele_offset + r->ref_start;
    const uint64_t *a1 = hap1 + (r->ref_start - start), *a2 = hap2 + (r->ref_start - start);
    for (int32_t i = lo; i < hi; i++) {
        const uint32_t o = ao[i] - first;
        t1 -= pool[o + a1[i]];
        t2 -= pool[o + a2[i]];
    }
    *x = t1 / 30.0; *y = t2 / 30.0;
}

/* stGenomeFragment_construct genomeFragment.c:40-69 (+ hmm.c:221-248) then
 * stGenomeFragment_refineGenomeFragment genomeFragment.c:165-232 */
void genome_fragment(const world *w, mrp_phase_result *g, const mrp_hmm *h, const uint64_t *chosen,
                            int64_t max_iterations) {
    const int64_t K = hmm_K(h);
    /* side[read]: 0 = unseen, 1 = reads1, 2 = reads2; first sighting along the path wins per set
     * (a read can be put in both sets by inconsistent columns; set semantics as in the reference) */
    uint8_t *in1 = xcalloc((size_t) w->n_reads + 1, 1), *in2 = xcalloc((size_t) w->n_reads + 1, 1);
    uint64_t *p = xmalloc(sizeof(uint64_t) * (size_t) K);
    uint64_t *scratch = xmalloc(sizeof(uint64_t) * 4 * (size_t) w->max_alleles);
    for (int64_t k = 0; k < K; k++) {
        p[k] = chosen[k]; /* partition of the traced-back cell of column k */
        const int32_t *cr = h->col_reads.a + h->read_off.a[k];
        for (int32_t i = 0; i < h->col_depth.a[k]; i++) {
            if ((p[k] >> i) & 1) { if (!in1[cr[i]]) { in1[cr[i]] = 1; g->reads1[g->n_reads1++] = cr[i]; } }
            else { if (!in2[cr[i]]) { in2[cr[i]] = 1; g->reads2[g->n_reads2++] = cr[i]; } }
        }
        fill_in_predicted_genome(w, g, h, k, p[k], scratch);
    }
    int64_t iteration = 0;
    uint8_t *m12 = xcalloc((size_t) w->n_reads + 1, 1), *m21 = xcalloc((size_t) w->n_reads + 1, 1);
    int32_t *n1 = xmalloc(sizeof(int32_t) * (size_t) (2 * w->n_reads + 2)), *n2 = xmalloc(sizeof(int32_t) * (size_t) (2 * w->n_reads + 2));
    while (iteration++ < max_iterations) {
        int64_t c12 = 0, c21 = 0;
        memset(m12, 0, (size_t) w->n_reads + 1); memset(m21, 0, (size_t) w->n_reads + 1);
        for (int64_t i = 0; i < g->n_reads1; i++) { /* :126-151 */
            const int32_t r = g->reads1[i];
            double x, y;
            read_log_prob2(w, g->haplotype_string1, g->haplotype_string2, g->ref_start, g->length, r, &x, &y);
            if (x < y) { m12[r] = 1; c12++; }
        }
        for (int64_t i = 0; i < g->n_reads2; i++) {
            const int32_t r = g->reads2[i];
            double x, y;
            read_log_prob2(w, g->haplotype_string1, g->haplotype_string2, g->ref_start, g->length, r, &x, &y);
            if (y < x) { m21[r] = 1; c21++; }
        }
        if (c12 + c21 == 0) break;
        int64_t a = 0, b = 0;
        for (int64_t i = 0; i < g->n_reads1; i++) if (!m12[g->reads1[i]]) n1[a++] = g->reads1[i];
        for (int64_t i = 0; i < g->n_reads2; i++) if (!m21[g->reads2[i]]) n2[b++] = g->reads2[i];
        for (int64_t i = 0; i < g->n_reads2; i++) if (m21[g->reads2[i]]) n1[a++] = g->reads2[i];
        for (int64_t i = 0; i < g->n_reads1; i++) if (m12[g->reads1[i]]) n2[b++] = g->reads1[i];
        memcpy(g->reads1, n1, sizeof(int32_t) * (size_t) a); memcpy(g->reads2, n2, sizeof(int32_t) * (size_t) b);
        g->n_reads1 = a; g->n_reads2 = b;
        for (int64_t k = 0; k < K; k++) { /* :211-226 */
            const int32_t *cr = h->col_reads.a + h->read_off.a[k];
            uint64_t flip = 0; /* (a read moved both ways -- it sat in both lists -- is flipped twice: not at all) */
            for (int32_t i = 0; i < h->col_depth.a[k]; i++) flip |= (uint64_t) (m12[cr[i]] ^ m21[cr[i]]) << i;
            if (!flip) continue; /* fillInPredictedGenome is a function of the column and its partition: unchanged */
            p[k] ^= flip;
            fill_in_predicted_genome(w, g, h, k, p[k], scratch);
        }
    }
    free(in1); free(in2); free(p); free(m12); free(m21); free(n1); free(n2); free(scratch);
}
/* bubbleGraph.c:2761-2779: genome fragment from the traced-back partitions, refinement, re-adding the filtered reads */
void finish_phase_parts(world *w, const mrp_hmm *hmm, const uint64_t *chosen, double fwd, double bwd, const mrp_params *params,
                               const int32_t *discarded, int64_t nd, mrp_phase_result **out) {
    mrp_phase_result *g = result_new(hmm->ref_start, hmm->ref_length, w->n_reads);
    genome_fragment(w, g, hmm, chosen, params->rounds_of_iterative_refinement); /* :2761-2764 */
    for (int64_t i = 0; i < nd; i++) { /* :2772-2779 */
        double x, y;
        read_log_prob2(w, g->haplotype_string1, g->haplotype_string2, g->ref_start, g->length, discarded[i], &x, &y);
        if (x < y) g->reads2[g->n_reads2++] = discarded[i]; else g->reads1[g->n_reads1++] = discarded[i];
    }
    g->hmm_forward = fwd; g->hmm_backward = bwd; g->n_sweeps = w->n_sweeps;
    *out = g;
}
