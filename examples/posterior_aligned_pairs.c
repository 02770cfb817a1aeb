/*
 * posterior_aligned_pairs.c -- the posterior half of the pairwise aligner from plain C, no Python:
 *
 *   (x, y) --mrp_posterior_tracebacks--> where the banded walk traces back          (pairwiseAligner.c:746-749, host only)
 *   (x, y) --mrp_posterior_aligned_pairs--> aligned pairs and gap pairs with weights  (getPosteriorProbsWithBanding, :706-844)
 *
 * on the pair of the reference's own test (AGCG against AGTTCG, tests/pairwiseAlignerTest.c:257-340) and on a longer pair with a
 * two-base deletion, with the nucleotide state machine of stateMachine3_constructNucleotide.  Prints every pair of the lists in the
 * order of generation (the reverse of what getAlignedPairsUsingAnchors returns, :1109-1111).
 *
 *   gcc -O2 -Iinclude examples/posterior_aligned_pairs.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o posterior_aligned_pairs
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

static void print_list(const char *name, const mrp_posterior_pairs *l, int64_t pair) {
    for (int64_t k = l->first[pair]; k < l->first[pair + 1]; k++)
        printf("%s %lld %d %d %d %a\n", name, (long long) pair, l->x[k], l->y[k], l->weight[k], l->log_posterior[k]);
}

int main(void) {
    /* stateMachine3_constructNucleotide (stateMachine.c:612-644) with the emissions of :409-432 */
    mrp_pair_hmm m = {-0.030064059121770816, -1.272871422049609, -1.272871422049609, -4.21256642, -4.21256642,
                      -0.3388262689231553, -0.3388262689231553, -4.910694825551255, -4.910694825551255, {0}, {0}, {0}};
    const double ma = -1.8917761142, tv = -4.3459578861, ti = -3.760242452;
    const double e[16] = {ma, tv, ti, tv, tv, ma, tv, ti, ti, tv, ma, tv, tv, ti, tv, ma};
    memcpy(m.e_match, e, sizeof(e));
    for (int i = 0; i < 4; i++) m.e_gap_x[i] = m.e_gap_y[i] = -1.3862943611;

    const char *xs[2] = {"AGCG", "ACGTTGCATGCCATTGACGGATCCGTAATG"};
    const char *ys[2] = {"AGTTCG", "ACGTTGCATGCCTGACGGATCCGTAATG"}; /* the second y lacks two bases of x */
    uint8_t pool[128];
    int64_t x_off[2], y_off[2], at = 0;
    int32_t x_len[2], y_len[2];
    for (int i = 0; i < 2; i++) {
        x_off[i] = at; x_len[i] = (int32_t) strlen(xs[i]);
        mrp_symbols_from_chars(xs[i], x_len[i], pool + at); at += x_len[i];
        y_off[i] = at; y_len[i] = (int32_t) strlen(ys[i]);
        mrp_symbols_from_chars(ys[i], y_len[i], pool + at); at += y_len[i];
    }

    /* a small band and frequent tracebacks, so that the longer pair has several: the reference's defaults are 20, 1000 and 40 */
    mrp_posterior_options opt = {0.2, 8, 12, 3, 0, 0, 1, 0};
    for (int i = 0; i < 2; i++) {
        int64_t triples[3 * 64], n_tb = 0;
        CHECK(mrp_posterior_tracebacks(NULL, 0, x_len[i], y_len[i], &opt, triples, 64, &n_tb));
        printf("tracebacks %d %lld:", i, (long long) n_tb);
        for (int64_t k = 0; k < n_tb && k < 64; k++) printf(" %lld,%lld,%lld", (long long) triples[3 * k], (long long) triples[3 * k + 1], (long long) triples[3 * k + 2]);
        printf("\n");
    }

    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    mrp_posterior_pairs match, gap_x, gap_y;
    double total[2];
    mrp_pairhmm_stats st;
    CHECK(mrp_posterior_aligned_pairs(ctx, &m, 1, 2, pool, at, x_off, x_len, y_off, y_len, NULL, NULL, NULL, &opt, &match, &gap_x, &gap_y, total, &st));
    for (int64_t i = 0; i < 2; i++) {
        printf("total %lld %a\n", (long long) i, total[i]);
        print_list("match", &match, i);
        print_list("gap_x", &gap_x, i);
        print_list("gap_y", &gap_y, i);
    }
    printf("%lld aligned pairs, %lld gap-x, %lld gap-y over %lld band cells\n", (long long) match.first[2], (long long) gap_x.first[2], (long long) gap_y.first[2],
           (long long) st.cells);
    mrp_posterior_pairs_free(&match);
    mrp_posterior_pairs_free(&gap_x);
    mrp_posterior_pairs_free(&gap_y);
    mrp_context_destroy(ctx);
    return 0;
}
