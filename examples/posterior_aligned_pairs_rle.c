/*
 * posterior_aligned_pairs_rle.c -- the pairwise aligner with run-length emissions, as margin polish runs it when
 * useRepeatCountsInAlignment is set (parser.c:510-524), from plain C, no Python:
 *
 *   chars --mrp_rle_compress--> symbols + repeat counts                          (rleString_construct, rle.c:7-38, and the count clamp)
 *   (x, y) + counts + table --mrp_forward_probabilities_rle--> log probability   (computeForwardProbability, pairwiseAligner.c:849-903)
 *   (x, y) + counts + table --mrp_posterior_aligned_pairs_rle--> aligned pairs   (getPosteriorProbsWithBanding, :706-844)
 *
 * on two strings that differ in the length of two homopolymer runs, with a small table that favours equal counts.  Prints the two
 * compressed strings, the forward probability, and the lists in the order of generation.
 *
 *   gcc -O2 -Iinclude examples/posterior_aligned_pairs_rle.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o posterior_aligned_pairs_rle
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

static void print_list(const char *name, const mrp_posterior_pairs *l) {
    for (int64_t k = l->first[0]; k < l->first[1]; k++) printf("%s %d %d %d %a\n", name, l->x[k], l->y[k], l->weight[k], l->log_posterior[k]);
}

int main(void) {
    /* stateMachine3_constructNucleotide (stateMachine.c:612-644) with the emissions of :409-432 */
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
    const mrp_repeat_model repeat = {R, 1, log_prob};

    const char *x = "ACCCGTTTTTTTTTTGCAATGGC", *y = "ACCGTTTTTTTTGCAATGGC"; /* x's run of ten T is clamped to 7 */
    uint8_t pool[64], counts[64];
    int64_t x_off = 0, y_off;
    const int32_t x_len = (int32_t) mrp_rle_compress(x, (int64_t) strlen(x), R, pool, counts);
    y_off = x_len;
    const int32_t y_len = (int32_t) mrp_rle_compress(y, (int64_t) strlen(y), R, pool + y_off, counts + y_off);
    if (x_len < 0 || y_len < 0) return 1;
    printf("x %d:", x_len);
    for (int i = 0; i < x_len; i++) printf(" %c%d", "ACGTN"[pool[i]], counts[i]);
    printf("\ny %d:", y_len);
    for (int i = 0; i < y_len; i++) printf(" %c%d", "ACGTN"[pool[y_off + i]], counts[y_off + i]);
    printf("\n");

    mrp_posterior_options opt = {0.01, 20, 1000, 40, 0, 0, 1, 0}; /* the reference's defaults, with gaps */
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    double forward = 0.0, total = 0.0;
    mrp_pairhmm_stats st;
    CHECK(mrp_forward_probabilities_rle(ctx, &m, &repeat, 1, 1, pool, counts, x_len + y_len, &x_off, &x_len, &y_off, &y_len, NULL, NULL, NULL, opt.expansion, 0, 0,
                                        &forward, &st));
    printf("forward %a\n", forward);
    mrp_posterior_pairs match, gap_x, gap_y;
    CHECK(mrp_posterior_aligned_pairs_rle(ctx, &m, &repeat, 1, 1, pool, counts, x_len + y_len, &x_off, &x_len, &y_off, &y_len, NULL, NULL, NULL, NULL, &opt, &match,
                                          &gap_x, &gap_y, &total, &st));
    printf("total %a\n", total);
    print_list("match", &match);
    print_list("gap_x", &gap_x);
    print_list("gap_y", &gap_y);
    printf("%lld aligned pairs over %lld band cells\n", (long long) (match.first[1] - match.first[0]), (long long) st.cells);
    mrp_posterior_pairs_free(&match);
    mrp_posterior_pairs_free(&gap_x);
    mrp_posterior_pairs_free(&gap_y);
    mrp_context_destroy(ctx);
    return forward == total ? 0 : 1;
}
