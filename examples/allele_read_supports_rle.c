/*
 * allele_read_supports_rle.c -- Bubble.alleleReadSupports as margin polish fills it when useRepeatCountsInAlignment is set
 * (bubbleGraph.c:1028-1075, :1193-1244), from plain C, no Python:
 *
 *   chars --mrp_rle_compress--> symbols + repeat counts                     (rleString_construct, rle.c:7-38, and the count clamp)
 *   bubbles + counts + two tables --mrp_allele_read_supports_rle--> floats  (the loop over a bubble's reads around computeForwardProbability)
 *
 * on one bubble of two alleles that differ in the length of a homopolymer run and four read substrings: the third repeats the first
 * on the other strand and copies its supports, the fourth is empty.  Short strings with small counts: every pair runs on the
 * pair-per-lane kernel.  Prints the compressed strings, then one line per (allele, read).
 *
 *   gcc -O2 -Iinclude examples/allele_read_supports_rle.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o allele_read_supports_rle
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "margin_rphmm.h"

#define CHECK(call)                                                                       \
    do {                                                                                  \
        int rc_ = (call);                                                                 \
        if (rc_ != MRP_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mrp_last_error()); return 1; } \
    } while (0)

#define R 8 /* max_repeat: counts 0..7 */
#define N_ALLELES 2
#define N_READS 4

int main(void) {
    /* stateMachine3_constructNucleotide (stateMachine.c:612-644) with the emissions of :409-432, for both strands */
    mrp_pair_hmm m = {-0.030064059121770816, -1.272871422049609, -1.272871422049609, -4.21256642, -4.21256642,
                      -0.3388262689231553, -0.3388262689231553, -4.910694825551255, -4.910694825551255, {0}, {0}, {0}};
    const double ma = -1.8917761142, tv = -4.3459578861, ti = -3.760242452;
    const double e[16] = {ma, tv, ti, tv, tv, ma, tv, ti, ti, tv, ma, tv, tv, ti, tv, ma};
    memcpy(m.e_match, e, sizeof(e));
    for (int i = 0; i < 4; i++) m.e_gap_x[i] = m.e_gap_y[i] = -1.3862943611;

    /* log10 probabilities [base][underlying][observed]: -0.05 for the same count, -0.6 * the difference otherwise, a little more for G and C */
    static double log_prob[4 * R * R];
    for (int b = 0; b < 4; b++)
        for (int u = 0; u < R; u++)
            for (int o = 0; o < R; o++) log_prob[(b * R + u) * R + o] = u == o ? -0.05 : -(0.6 + 0.05 * (b == 1 || b == 2)) * abs(u - o);
    const mrp_repeat_model forward_repeat = {R, 1, log_prob}, reverse_repeat = {R, 0, log_prob};

    const char *alleles[N_ALLELES] = {"ACCCGTTTTTGCAATGGC", "ACCCGTTTGCAATGGC"};
    const char *reads[N_READS] = {"ACCCGTTTTGCAATGGC", "ACCGTTTTTGCATGGC", "ACCCGTTTTGCAATGGC", ""};
    const uint8_t read_forward_strand[N_READS] = {1, 0, 0, 1};
    uint8_t pool[256], counts[256];
    int64_t allele_off[N_ALLELES], read_off[N_READS], at = 0;
    int32_t allele_len[N_ALLELES], read_len[N_READS];
    for (int k = 0; k < N_ALLELES + N_READS; k++) {
        const char *s = k < N_ALLELES ? alleles[k] : reads[k - N_ALLELES];
        const int64_t n = mrp_rle_compress(s, (int64_t) strlen(s), R, pool + at, counts + at);
        if (n < 0) return 1;
        printf("%s %d %lld:", k < N_ALLELES ? "allele" : "read", k < N_ALLELES ? k : k - N_ALLELES, (long long) n);
        for (int64_t i = 0; i < n; i++) printf(" %c%d", "ACGTN"[pool[at + i]], counts[at + i]);
        printf("\n");
        if (k < N_ALLELES) { allele_off[k] = at; allele_len[k] = (int32_t) n; }
        else { read_off[k - N_ALLELES] = at; read_len[k - N_ALLELES] = (int32_t) n; }
        at += n;
    }
    const int64_t allele_first[2] = {0, N_ALLELES}, read_first[2] = {0, N_READS};

    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    float support[N_ALLELES * N_READS];
    mrp_pairhmm_stats st;
    CHECK(mrp_allele_read_supports_rle(ctx, &m, &m, &forward_repeat, &reverse_repeat, 1, allele_first, read_first, pool, counts, at, allele_off, allele_len, read_off,
                                       read_len, read_forward_strand, 20, support, &st));
    for (int j = 0; j < N_ALLELES; j++)
        for (int k = 0; k < N_READS; k++) printf("support %d %d %a\n", j, k, (double) support[j * N_READS + k]);
    printf("%lld pairs a lane, %lld pairs a wave, %lld cells\n", (long long) st.pairs_lane, (long long) st.pairs_wave, (long long) st.cells);
    mrp_context_destroy(ctx);
    return 0;
}
