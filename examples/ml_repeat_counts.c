/*
 * ml_repeat_counts.c -- from a draft consensus and its reads to the polished sequence, as margin polish ends a chunk
 * (poa_estimateRepeatCountsUsingBayesianModel, poa.c:1715-1727, then rleString_expand), from plain C, no Python:
 *
 *   chars --mrp_rle_compress--> symbols + run lengths                            (rleString_construct, rle.c:7-38)
 *   (consensus, read) --mrp_posterior_aligned_pairs_rle--> matches               (getPosteriorProbsWithBanding, pairwiseAligner.c:706-844)
 *   consensus + run lengths + matches --mrp_ml_repeat_counts--> a count per node (repeatSubMatrix_getMLRepeatCount, repeatSubMatrix.c:124-143)
 *   symbols + counts --mrp_rle_expand--> chars                                   (rleString_expand, rle.c:145-155)
 *
 * The alignment reads counts clamped below max_repeat (mrp_rle_compress with R); the estimate reads the run lengths saturated at 255
 * (mrp_rle_compress with 256), so that an overlong run is treated as the reference treats it.  Reads 1 and 3 lie on the reverse strand.
 * Prints the compressed draft, every node's count with its log probability, and the polished sequence.
 *
 *   gcc -O2 -Iinclude examples/ml_repeat_counts.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o ml_repeat_counts
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
#define N_READS 5

int main(void) {
    /* stateMachine3_constructNucleotide (stateMachine.c:612-644) with the emissions of :409-432, and its reverse complement */
    mrp_pair_hmm models[2] = {{-0.030064059121770816, -1.272871422049609, -1.272871422049609, -4.21256642, -4.21256642,
                               -0.3388262689231553, -0.3388262689231553, -4.910694825551255, -4.910694825551255, {0}, {0}, {0}}};
    const double ma = -1.8917761142, tv = -4.3459578861, ti = -3.760242452;
    const double e[16] = {ma, tv, ti, tv, tv, ma, tv, ti, ti, tv, ma, tv, tv, ti, tv, ma};
    memcpy(models[0].e_match, e, sizeof(e));
    for (int i = 0; i < 4; i++) models[0].e_gap_x[i] = models[0].e_gap_y[i] = -1.3862943611;
    models[1] = models[0];
    mrp_pair_hmm_reverse_complement(&models[1]);

    /* log10 probabilities [base][underlying][observed]: -0.05 for the same count, -0.6 * the difference otherwise, a little more for G and C */
    static double log_prob[4 * R * R];
    for (int b = 0; b < 4; b++)
        for (int u = 0; u < R; u++)
            for (int o = 0; o < R; o++) log_prob[(b * R + u) * R + o] = u == o ? -0.05 : -(0.6 + 0.05 * (b == 1 || b == 2)) * abs(u - o);
    const mrp_repeat_model repeat[2] = {{R, 1, log_prob}, {R, 0, log_prob}};

    const char *draft = "ACCGTTTTTGCAATGGC";
    const char *reads[N_READS] = {"ACCCGTTTTTTGCAATGGGC", "ACCCGTTTTTTGCAATGGC", "ACCCGTTTTTGCAATGGGC", "ACCGTTTTTTGCAATGGGC", "ACCCGTTTTTTGCAAATGGGC"};
    const uint8_t strand[N_READS] = {1, 0, 1, 0, 1};

    uint8_t pool[256], clamped[256], lengths[256];
    int64_t x_off[N_READS], y_off[N_READS], at;
    int32_t x_len[N_READS], y_len[N_READS];
    uint8_t model_index[N_READS];
    const int32_t n_nodes = (int32_t) mrp_rle_compress(draft, (int64_t) strlen(draft), R, pool, clamped);
    if (n_nodes < 0 || mrp_rle_compress(draft, (int64_t) strlen(draft), 256, pool, lengths) != n_nodes) return 1;
    at = n_nodes;
    for (int r = 0; r < N_READS; r++) {
        const int64_t n = mrp_rle_compress(reads[r], (int64_t) strlen(reads[r]), R, pool + at, clamped + at);
        if (n < 0 || mrp_rle_compress(reads[r], (int64_t) strlen(reads[r]), 256, pool + at, lengths + at) != n) return 1;
        x_off[r] = 0; x_len[r] = n_nodes; y_off[r] = at; y_len[r] = (int32_t) n;
        model_index[r] = strand[r] ? 0 : 1;
        at += n;
    }
    printf("draft %d:", n_nodes);
    for (int i = 0; i < n_nodes; i++) printf(" %c%d", "ACGTN"[pool[i]], lengths[i]);
    printf("\n");

    mrp_posterior_options popt = {0.01, 20, 1000, 40, 0, 0, 0, 0}; /* the reference's defaults, matches only */
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    mrp_posterior_pairs match;
    CHECK(mrp_posterior_aligned_pairs_rle(ctx, models, repeat, 2, N_READS, pool, clamped, at, x_off, x_len, y_off, y_len, model_index, NULL, NULL, NULL, &popt,
                                          &match, NULL, NULL, NULL, NULL));

    /* one consensus: all nodes, all reads; the matches as they came, walked backwards (the order poa_augment receives) */
    const int64_t node_first[2] = {0, n_nodes}, read_first[2] = {0, N_READS};
    const mrp_repeat_count_options opt = {1, 0, 0.0, 0};
    int32_t count[64];
    double lp[64];
    int64_t length = 0;
    mrp_repeat_count_stats st;
    CHECK(mrp_ml_repeat_counts(ctx, log_prob, R, 1, node_first, pool, read_first, lengths, at, y_off, y_len, strand, NULL, NULL, &match, &opt, count, lp, &length,
                               &st));
    for (int i = 0; i < n_nodes; i++) printf("node %d %c %d %a\n", i, "ACGTN"[pool[i]], count[i], lp[i]);

    char polished[512];
    const int64_t n = mrp_rle_expand(pool, NULL, count, n_nodes, polished, (int64_t) sizeof(polished) - 1);
    if (n != length) return 1;
    polished[n] = '\0';
    printf("polished %s\n", polished);
    printf("%lld observations of %lld nodes, %lld candidates\n", (long long) st.observations, (long long) st.nodes_observed, (long long) st.candidates);
    mrp_posterior_pairs_free(&match);
    mrp_context_destroy(ctx);
    return 0;
}
