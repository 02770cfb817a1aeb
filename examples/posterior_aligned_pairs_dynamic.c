/*
 * posterior_aligned_pairs_dynamic.c -- the posterior half of the pairwise aligner the way margin's shipped parameters call it, from
 * plain C, no Python:
 *
 *   anchors (x, y, expansion) --mrp_band_diagonals_dynamic--> the band of band_constructDynamic   (pairwiseAligner.c:120-173, host only)
 *   (x, y) + anchors --mrp_posterior_aligned_pairs_dynamic--> aligned pairs and gap pairs          (getPosteriorProbsWithBanding with
 *                                                                                                  dynamicAnchorExpansion, :726)
 *
 * on one anchored pair whose anchors carry different expansions, and on one unanchored pair of 2 100 symbols, whose widest diagonal
 * holds more than 2 048 cells: refused until mrp_context_set_posterior_wide_pairs is on.  Prints the first pair's lists in the order
 * of generation and the second pair's counts with its first entries.
 *
 *   gcc -O2 -Iinclude examples/posterior_aligned_pairs_dynamic.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o posterior_aligned_pairs_dynamic
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

#define WIDE 2100

static void print_list(const char *name, const mrp_posterior_pairs *l, int64_t pair, int64_t at_most) {
    for (int64_t k = l->first[pair]; k < l->first[pair + 1] && k < l->first[pair] + at_most; k++)
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

    /* pair 0: y lacks two bases of x between the second and the third anchor, which therefore gets the widest expansion */
    const char *x0 = "ACGTTGCATGCCATTGACGGATCCGTAATG", *y0 = "ACGTTGCATGCCTGACGGATCCGTAATG";
    const int64_t anchors[6] = {3, 3, 9, 9, 20, 18};
    const int64_t anchor_expansion[3] = {2, 0, 6};
    const int64_t anchor_off[3] = {0, 3, 3}; /* pair 1 has no anchors: its band is its whole matrix */
    static uint8_t pool[64 + 2 * WIDE + 16];
    int64_t x_off[2], y_off[2], at = 0;
    int32_t x_len[2], y_len[2];
    x_off[0] = at; x_len[0] = (int32_t) strlen(x0); mrp_symbols_from_chars(x0, x_len[0], pool + at); at += x_len[0];
    y_off[0] = at; y_len[0] = (int32_t) strlen(y0); mrp_symbols_from_chars(y0, y_len[0], pool + at); at += y_len[0];
    /* pair 1: WIDE symbols from a small generator; y is x with every 97th symbol changed and every 211th left out */
    uint32_t lcg = 12345;
    x_off[1] = at; x_len[1] = WIDE;
    for (int i = 0; i < WIDE; i++) { lcg = lcg * 1664525u + 1013904223u; pool[at++] = (uint8_t) (lcg >> 30); }
    y_off[1] = at; y_len[1] = 0;
    for (int i = 0; i < WIDE; i++) {
        if (i % 211 == 210) continue;
        pool[at++] = (uint8_t) (i % 97 == 96 ? (pool[x_off[1] + i] + 1) & 3 : pool[x_off[1] + i]);
        y_len[1]++;
    }

    int32_t lo[64], hi[64], width = 0;
    int64_t cells = 0;
    CHECK(mrp_band_diagonals_dynamic(anchors, 3, x_len[0], y_len[0], anchor_expansion, lo, hi));
    printf("band 0:");
    for (int d = 0; d <= x_len[0] + y_len[0]; d++) printf(" %d..%d", lo[d], hi[d]);
    printf("\n");
    CHECK(mrp_pair_diagonal_width_dynamic(NULL, 0, x_len[1], y_len[1], NULL, &width, &cells));
    printf("pair 1: widest diagonal %d cells, %lld band cells\n", width, (long long) cells);

    /* the reference's defaults (threshold 0.01, diagonalExpansion 20, a traceback every 1000 diagonals, 40 kept), with gaps */
    mrp_posterior_options opt = {0.01, 20, 1000, 40, 0, 0, 1, 0};
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    mrp_posterior_pairs match, gap_x, gap_y;
    double total[2];
    mrp_pairhmm_stats st;
    int rc = mrp_posterior_aligned_pairs_dynamic(ctx, &m, 1, 2, pool, at, x_off, x_len, y_off, y_len, NULL, anchor_off, anchors, anchor_expansion, &opt, &match,
                                                 &gap_x, &gap_y, total, &st);
    printf("switch off: %d (%s)\n", rc, rc == MRP_OK ? "ran" : mrp_last_error());
    if (rc == MRP_OK) return 1; /* pair 1 must have been refused */
    CHECK(mrp_context_set_posterior_wide_pairs(ctx, 1));
    CHECK(mrp_posterior_aligned_pairs_dynamic(ctx, &m, 1, 2, pool, at, x_off, x_len, y_off, y_len, NULL, anchor_off, anchors, anchor_expansion, &opt, &match, &gap_x,
                                              &gap_y, total, &st));
    int64_t wide_pairs = 0, wide_cells = 0;
    CHECK(mrp_context_posterior_wide_count(ctx, &wide_pairs, &wide_cells));
    printf("total 0 %a\n", total[0]);
    print_list("match", &match, 0, 1 << 30);
    print_list("gap_x", &gap_x, 0, 1 << 30);
    print_list("gap_y", &gap_y, 0, 1 << 30);
    printf("total 1 %a: %lld aligned pairs, %lld gap-x, %lld gap-y; the first of each:\n", total[1], (long long) (match.first[2] - match.first[1]),
           (long long) (gap_x.first[2] - gap_x.first[1]), (long long) (gap_y.first[2] - gap_y.first[1]));
    print_list("match", &match, 1, 5);
    print_list("gap_x", &gap_x, 1, 5);
    print_list("gap_y", &gap_y, 1, 5);
    printf("%lld band cells in all; the pair-per-workgroup kernels took %lld pair with %lld of them\n", (long long) st.cells, (long long) wide_pairs,
           (long long) wide_cells);
    mrp_posterior_pairs_free(&match);
    mrp_posterior_pairs_free(&gap_x);
    mrp_posterior_pairs_free(&gap_y);
    mrp_context_destroy(ctx);
    return 0;
}
