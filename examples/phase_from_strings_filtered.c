/*
 * phase_from_strings_filtered.c -- front and back half of margin phase's chunk loop (phase.c:395-436) from plain C in ONE call:
 *
 *   primary reads' substrings x alleles ------+
 *   filtered reads' substrings at the bubbles +--mrp_phase_string_chunks_with_filtered--> haplotypes, HP tags of the primary reads,
 *   filtered variants and their entries ------+     HP tags of the filtered and the untagged primary reads, phase of the variants
 *
 * on a synthetic chunk (two haplotypes that differ at every site, noisy reads, every second read "filtered").  Prints how many
 * filtered reads were tagged and agree with the haplotype they were drawn from, and how many variants were phased.  With a file
 * name as its argument it also writes the inputs and the results there, one record per line (tests/test_c_example_filtered.py
 * replays them through the chain of single calls).
 *
 *   gcc -O2 -Iinclude examples/phase_from_strings_filtered.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o phase_filtered
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "margin_rphmm.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { /* xorshift64* */
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t) ((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static double uni(void) { return rnd() / 4294967296.0; }

#define CHECK(call)                                                                       \
    do {                                                                                  \
        int rc_ = (call);                                                                 \
        if (rc_ != MRP_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mrp_last_error()); return 1; } \
    } while (0)

enum { N_SITES = 80, N_READS = 160, N_VARIANTS = 12, FLANK = 12, LA = 2 * FLANK + 1, MAX_SUB = LA + 8 };

/* a noisy copy of src (3 % substitutions, 1 % deletions, 1 % insertions) appended to pool; returns its length */
static int noisy(const uint8_t *src, uint8_t *dst) {
    int n = 0;
    for (int i = 0; i < LA; i++) {
        const double u = uni();
        if (u < 0.01) continue;
        dst[n++] = u < 0.04 ? (uint8_t) (rnd() & 3) : src[i];
        if (uni() < 0.01 && n < MAX_SUB) dst[n++] = (uint8_t) (rnd() & 3);
    }
    return n;
}

static void dump_symbols(FILE *f, const uint8_t *s, int n) {
    for (int i = 0; i < n; i++) fputc("ACGT"[s[i] & 3], f);
    fputc('\n', f);
}

int main(int argc, char **argv) {
    FILE *dump = argc > 1 ? fopen(argv[1], "w") : NULL;
    if (argc > 1 && !dump) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));

    /* the state machine of the shipped parameter file (params/base_params.json, hmmForwardStrandReadGivenReference) */
    mrp_pair_hmm fwd;
    const double tr[9] = {0.8, 0.1, 0.1, 0.5, 0.5, 0.0, 0.5, 0.0, 0.5};
    const double em[16] = {0.969, 0.005, 0.017, 0.009, 0.008, 0.973, 0.007, 0.012, 0.021, 0.007, 0.967, 0.006, 0.008, 0.008, 0.004, 0.98};
    fwd.match_continue = log(tr[0]);
    fwd.match_from_gap_x = fwd.match_from_gap_y = log((tr[3] + tr[6]) / 2.0);
    fwd.gap_open_x = fwd.gap_open_y = log((tr[1] + tr[2]) / 2.0);
    fwd.gap_extend_x = fwd.gap_extend_y = log((tr[4] + tr[8]) / 2.0);
    fwd.gap_switch_to_x = fwd.gap_switch_to_y = log((tr[7] + tr[5]) / 2.0); /* log 0 = -inf */
    for (int i = 0; i < 16; i++) fwd.e_match[i] = log(em[i]);
    for (int i = 0; i < 4; i++) { fwd.e_gap_x[i] = log(1.0); fwd.e_gap_y[i] = log(0.25); }
    mrp_pair_hmm rev = fwd;
    mrp_pair_hmm_reverse_complement(&rev);

    /* reads: a span of sites, a haplotype, a strand; every second read is a filtered one.  index[r]: among its kind */
    int span0[N_READS], span1[N_READS], hap[N_READS], filtered[N_READS], index[N_READS], n_primary = 0, n_filtered = 0;
    uint8_t strand_p[N_READS], strand_f[N_READS];
    for (int r = 0; r < N_READS; r++) {
        span0[r] = (int) (rnd() % (N_SITES - 5));
        span1[r] = r % 16 == 0 ? span0[r] : span0[r] + 1 + (int) (rnd() % 30); /* every eighth primary read covers one site only */
        if (span1[r] >= N_SITES) span1[r] = N_SITES - 1;
        hap[r] = (int) (rnd() & 1);
        filtered[r] = r & 1;
        const uint8_t st = (uint8_t) (rnd() & 1);
        if (filtered[r]) { index[r] = n_filtered; strand_f[n_filtered++] = st; }
        else { index[r] = n_primary; strand_p[n_primary++] = st; }
    }
    /* the chunk: two alleles per bubble, the primary reads' substrings; the rest: the filtered reads' substrings at the same bubbles */
    const size_t per_site = (size_t) N_READS * MAX_SUB + 4 * LA;
    uint8_t *pool = malloc(N_SITES * per_site), *rpool = malloc((N_SITES + N_VARIANTS) * per_site);
    int64_t pool_n = 0, rpool_n = 0, n_subs = 0, n_fsubs = 0;
    int64_t allele_first[N_SITES + 1], sub_first[N_SITES + 1], fsub_first[N_SITES + 1], allele_off[2 * N_SITES];
    int32_t allele_len[2 * N_SITES];
    int64_t *sub_off = malloc(sizeof(int64_t) * N_SITES * N_READS), *fsub_off = malloc(sizeof(int64_t) * N_SITES * N_READS);
    int32_t *sub_len = malloc(sizeof(int32_t) * N_SITES * N_READS), *sub_read = malloc(sizeof(int32_t) * N_SITES * N_READS);
    int32_t *fsub_len = malloc(sizeof(int32_t) * N_SITES * N_READS), *fsub_read = malloc(sizeof(int32_t) * N_SITES * N_READS);
    int truth[N_SITES];
    if (dump) {
        const double *m[2] = {(const double *) &fwd, (const double *) &rev}; /* the two state machines, every field a double */
        for (int k = 0; k < 2; k++) {
            fprintf(dump, k ? "model_r" : "model_f");
            for (size_t i = 0; i < sizeof(mrp_pair_hmm) / sizeof(double); i++) fprintf(dump, " %a", m[k][i]);
            fprintf(dump, "\n");
        }
        fprintf(dump, "reads %d %d\nstrand_p", n_primary, n_filtered);
        for (int r = 0; r < n_primary; r++) fprintf(dump, " %d", strand_p[r]);
        fprintf(dump, "\nstrand_f");
        for (int r = 0; r < n_filtered; r++) fprintf(dump, " %d", strand_f[r]);
        fprintf(dump, "\n");
    }
    for (int s = 0; s < N_SITES; s++) {
        uint8_t ref[LA], alt[LA];
        for (int i = 0; i < LA; i++) ref[i] = alt[i] = (uint8_t) (rnd() & 3);
        alt[FLANK] = (uint8_t) ((alt[FLANK] + 1 + rnd() % 3) & 3);
        truth[s] = (int) (rnd() & 1); /* allele of haplotype 0 */
        allele_first[s] = 2 * s;
        sub_first[s] = n_subs;
        fsub_first[s] = n_fsubs;
        if (dump) fprintf(dump, "bubble\n");
        for (int a = 0; a < 2; a++) {
            allele_off[2 * s + a] = pool_n;
            allele_len[2 * s + a] = LA;
            memcpy(pool + pool_n, a ? alt : ref, LA);
            if (dump) { fprintf(dump, "a "); dump_symbols(dump, pool + pool_n, LA); }
            pool_n += LA;
        }
        for (int r = 0; r < N_READS; r++) {
            if (s < span0[r] || s > span1[r]) continue;
            const uint8_t *src = (hap[r] == 0 ? truth[s] : 1 - truth[s]) ? alt : ref;
            if (filtered[r]) {
                fsub_off[n_fsubs] = rpool_n;
                fsub_len[n_fsubs] = noisy(src, rpool + rpool_n);
                fsub_read[n_fsubs] = index[r];
                if (dump) { fprintf(dump, "f %d ", index[r]); dump_symbols(dump, rpool + rpool_n, fsub_len[n_fsubs]); }
                rpool_n += fsub_len[n_fsubs++];
            } else {
                sub_off[n_subs] = pool_n;
                sub_len[n_subs] = noisy(src, pool + pool_n);
                sub_read[n_subs] = index[r];
                if (dump) { fprintf(dump, "p %d ", index[r]); dump_symbols(dump, pool + pool_n, sub_len[n_subs]); }
                pool_n += sub_len[n_subs++];
            }
        }
    }
    allele_first[N_SITES] = 2 * N_SITES;
    sub_first[N_SITES] = n_subs;
    fsub_first[N_SITES] = n_fsubs;
    /* filtered variants: three alleles at a site of the chunk, genotype (1, 2) or (2, 1) along the two haplotypes, an entry per
     * spanning read, primary or filtered, in read order */
    int64_t valle_first[N_VARIANTS + 1], ventry_first[N_VARIANTS + 1], valle_off[3 * N_VARIANTS], n_ventries = 0;
    int32_t valle_len[3 * N_VARIANTS], gt[2 * N_VARIANTS];
    int64_t *ventry_off = malloc(sizeof(int64_t) * N_VARIANTS * N_READS);
    int32_t *ventry_len = malloc(sizeof(int32_t) * N_VARIANTS * N_READS), *ventry_read = malloc(sizeof(int32_t) * N_VARIANTS * N_READS);
    for (int v = 0; v < N_VARIANTS; v++) {
        const int s = (int) (rnd() % N_SITES);
        uint8_t al[3][LA];
        for (int i = 0; i < LA; i++) al[0][i] = al[1][i] = al[2][i] = (uint8_t) (rnd() & 3);
        al[1][FLANK] = (uint8_t) ((al[0][FLANK] + 1) & 3);
        al[2][FLANK - 3] = (uint8_t) ((al[0][FLANK - 3] + 2) & 3);
        gt[2 * v] = (rnd() & 1) ? 1 : 2;
        gt[2 * v + 1] = 3 - gt[2 * v];
        valle_first[v] = 3 * v;
        ventry_first[v] = n_ventries;
        if (dump) fprintf(dump, "variant %d %d\n", gt[2 * v], gt[2 * v + 1]);
        for (int a = 0; a < 3; a++) {
            valle_off[3 * v + a] = rpool_n;
            valle_len[3 * v + a] = LA;
            memcpy(rpool + rpool_n, al[a], LA);
            if (dump) { fprintf(dump, "a "); dump_symbols(dump, al[a], LA); }
            rpool_n += LA;
        }
        for (int r = 0; r < N_READS; r++) {
            if (s < span0[r] || s > span1[r]) continue;
            ventry_off[n_ventries] = rpool_n;
            ventry_len[n_ventries] = noisy(al[gt[2 * v + hap[r]]], rpool + rpool_n);
            ventry_read[n_ventries] = filtered[r] ? n_primary + index[r] : index[r];
            if (dump) { fprintf(dump, "e %d ", ventry_read[n_ventries]); dump_symbols(dump, rpool + rpool_n, ventry_len[n_ventries]); }
            rpool_n += ventry_len[n_ventries++];
        }
    }
    valle_first[N_VARIANTS] = 3 * N_VARIANTS;
    ventry_first[N_VARIANTS] = n_ventries;

    static char name_buf[N_READS][16];
    const char *names[N_READS]; /* read ids: they order hmms that share start and length (hmm.c:82-87) */
    for (int r = 0; r < n_primary; r++) { snprintf(name_buf[r], sizeof(name_buf[r]), "read%04d", r); names[r] = name_buf[r]; }
    const mrp_string_chunk chunk = {N_SITES, n_primary, pool, pool_n, allele_first, allele_off, allele_len, sub_first, sub_off, sub_len, sub_read, names, strand_p};
    const mrp_string_chunk_rest rest = {n_filtered, strand_f, rpool, rpool_n, fsub_first, fsub_off, fsub_len, fsub_read,
                                        N_VARIANTS, valle_first, valle_off, valle_len, gt, ventry_first, ventry_read, ventry_off, ventry_len};

    /* the one call: min_phred 30 leaves the primary reads over a single site untagged; they are tagged with the filtered ones */
    mrp_params params = {1, 1, 1, 0, 100, 100, 0.0, 64, 2, 10}; /* params/base_params.json "phase" */
    mrp_phase_result *res[1] = {NULL};
    int8_t *tag = malloc((size_t) n_primary);
    int8_t *tags[1] = {tag};
    mrp_filtered_out out;
    mrp_string_filtered_stats st;
    CHECK(mrp_phase_string_chunks_with_filtered(ctx, 1, &chunk, &rest, &fwd, &rev, 4, 512, 0.0, &params, 30, res, tags, NULL, NULL, &out, &st));

    int64_t f_tagged = 0, f_agree = 0, p_agree = 0, p_tagged = 0, phased = 0;
    for (int r = 0; r < N_READS; r++) {
        const int32_t h = out.read_hap[filtered[r] ? n_primary + index[r] : index[r]];
        if (h != 1 && h != 2) continue;
        if (filtered[r]) { f_tagged++; f_agree += (h - 1) == hap[r]; }
        else { p_tagged++; p_agree += (h - 1) == hap[r]; }
    }
    if (2 * p_agree < p_tagged) { p_agree = p_tagged - p_agree; f_agree = f_tagged - f_agree; } /* the global label */
    for (int v = 0; v < N_VARIANTS; v++) phased += out.variant_state[v] == MRP_VARIANT_CIS || out.variant_state[v] == MRP_VARIANT_TRANS;
    printf("%s: %lld pairs in one launch (%lld only for the back half, %lld of them read), resident=%d; %lld of %d filtered reads tagged, %lld agree "
           "with their haplotype; %lld of %d filtered variants phased\n",
           mrp_version(), (long long) st.pairs_scored, (long long) st.pairs_speculative, (long long) st.pairs_read_by_results, st.chunks.phase.resident,
           (long long) f_tagged, n_filtered, (long long) f_agree, (long long) phased, N_VARIANTS);
    if (dump) {
        fprintf(dump, "read_hap");
        for (int64_t r = 0; r < out.n_reads; r++) fprintf(dump, " %d", out.read_hap[r]);
        fprintf(dump, "\nh1");
        for (int64_t r = 0; r < out.n_reads; r++) fprintf(dump, " %a", out.h1[r]);
        fprintf(dump, "\nh2");
        for (int64_t r = 0; r < out.n_reads; r++) fprintf(dump, " %a", out.h2[r]);
        fprintf(dump, "\nvariant_state");
        for (int64_t v = 0; v < out.n_variants; v++) fprintf(dump, " %d", out.variant_state[v]);
        fprintf(dump, "\ncis");
        for (int64_t v = 0; v < out.n_variants; v++) fprintf(dump, " %a", out.cis[v]);
        fprintf(dump, "\ntrans");
        for (int64_t v = 0; v < out.n_variants; v++) fprintf(dump, " %a", out.trans[v]);
        fprintf(dump, "\n");
        fclose(dump);
    }
    const int ok = f_tagged * 10 >= n_filtered * 8 && f_agree * 10 >= f_tagged * 9 && phased * 10 >= N_VARIANTS * 8;

    mrp_phase_result_destroy(res[0]);
    mrp_free(out.read_hap); mrp_free(out.h1); mrp_free(out.h2); mrp_free(out.variant_state); mrp_free(out.cis); mrp_free(out.trans);
    free(tag); free(pool); free(rpool); free(sub_off); free(sub_len); free(sub_read); free(fsub_off); free(fsub_len); free(fsub_read);
    free(ventry_off); free(ventry_len); free(ventry_read);
    mrp_context_destroy(ctx);
    (void) truth;
    return ok ? 0 : 2;
}
