/*
 * poa_consensus.c -- one round of margin polish's realignment for one chunk (poa_realign, poa.c:668-716, then poa_getConsensus,
 * :1350-1588), from plain C, no Python:
 *
 *   chars --mrp_rle_compress--> symbols + run lengths                                     (rleString_construct, rle.c:7-38)
 *   (consensus, read) --mrp_posterior_aligned_pairs_rle(with_gaps = 1)--> three lists     (getPosteriorProbsWithBanding, pairwiseAligner.c:706-844)
 *   matches, gap-x = deletes, gap-y = inserts --mrp_poa_augment--> weights, inserts, deletes, picks (poa_augment, poa.c:317-543)
 *   the graph --mrp_poa_consensus--> the new consensus as run-length symbols              (poa_getConsensus)
 *   symbols + counts --mrp_rle_expand--> chars                                            (rleString_expand, rle.c:145-155)
 *
 * The alignment reads counts clamped below max_repeat (mrp_rle_compress with R); the graph reads the reads' run lengths saturated at 255
 * (mrp_rle_compress with 256) and the consensus' clamped ones (a reference count must lie below max_repeat).  Reads 1 and 3 lie on the
 * reverse strand.  The draft lacks a G that every read has and has TT where every read has T.  Prints the compressed draft, every node with
 * its picks, inserts and deletes, the totals and the new sequence.
 *
 *   gcc -O2 -Iinclude examples/poa_consensus.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o poa_consensus
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

    const char *draft = "ACCGTTTTTCAATTGGC";
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

    mrp_posterior_options popt = {0.01, 20, 1000, 40, 0, 0, 1, 0}; /* the reference's defaults, with the gap lists */
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    mrp_posterior_pairs match, gap_x, gap_y;
    CHECK(mrp_posterior_aligned_pairs_rle(ctx, models, repeat, 2, N_READS, pool, clamped, at, x_off, x_len, y_off, y_len, model_index, NULL, NULL, NULL, &popt,
                                          &match, &gap_x, &gap_y, NULL, NULL));

    /* one consensus: all positions, all reads; gap-x are the deletes, gap-y the inserts */
    const int64_t node_first[2] = {0, n_nodes}, read_first[2] = {0, N_READS};
    const mrp_poa_options opt = {1, 1, 0.5, 0, 0, 0};
    mrp_poa poa;
    mrp_poa_stats st;
    CHECK(mrp_poa_augment(ctx, R, 1, node_first, pool, clamped, read_first, pool, lengths, at, y_off, y_len, strand, NULL, &match, &gap_x, &gap_y, &opt, &poa, &st));
    for (int64_t k = 0; k < poa.n_nodes; k++) {
        printf("node %lld %c pick %c %d weights", (long long) k, k ? "ACGTN"[pool[k - 1]] : 'N', "ACGTN"[poa.base_pick[k]], poa.repeat_count_pick[k]);
        for (int j = 0; j < 5; j++) printf(" %.0f", poa.base_weight[5 * k + j]);
        for (int64_t j = poa.insert_first[k]; j < poa.insert_first[k + 1]; j++) {
            printf(" +");
            for (int32_t q = 0; q < poa.insert_str_len[j]; q++)
                printf("%c%d", "ACGTN"[poa.pool_symbols[poa.insert_str_off[j] + q]], poa.pool_counts[poa.insert_str_off[j] + q]);
            printf(":%.0f/%.0f", poa.insert_weight_forward[j], poa.insert_weight_reverse[j]);
        }
        for (int64_t j = poa.delete_first[k]; j < poa.delete_first[k + 1]; j++)
            printf(" -%d:%.0f/%.0f", poa.delete_length[j], poa.delete_weight_forward[j], poa.delete_weight_reverse[j]);
        printf("\n");
    }
    printf("totals %.0f %.0f %.0f %.0f\n", poa.totals[0], poa.totals[1], poa.totals[2], poa.totals[3]);

    uint8_t *symbols = NULL;
    int32_t *counts = NULL;
    int64_t length = 0, *map = NULL;
    CHECK(mrp_poa_consensus(n_nodes, poa.base_weight, poa.base_pick, poa.repeat_count_pick, poa.insert_first, poa.insert_str_off, poa.insert_str_len,
                            poa.insert_weight_forward, poa.insert_weight_reverse, poa.pool_symbols, poa.pool_counts, poa.pool_len, poa.delete_first,
                            poa.delete_length, poa.delete_weight_forward, poa.delete_weight_reverse, 1, &symbols, &counts, &length, &map));
    printf("map");
    for (int i = 0; i < n_nodes; i++) printf(" %lld", (long long) map[i]);
    printf("\n");
    char polished[512];
    const int64_t n = mrp_rle_expand(symbols, NULL, counts, length, polished, (int64_t) sizeof(polished) - 1);
    if (n < 0) return 1;
    polished[n] = '\0';
    printf("consensus %s\n", polished);
    printf("%lld matches, %lld deletes, %lld inserts: %lld complete inserts (%lld distinct), %lld complete deletes (%lld distinct)\n", (long long) st.matches,
           (long long) st.deletes, (long long) st.inserts, (long long) st.complete_inserts, (long long) st.distinct_inserts, (long long) st.complete_deletes,
           (long long) st.distinct_deletes);
    mrp_free(symbols);
    mrp_free(counts);
    mrp_free(map);
    mrp_poa_free(&poa);
    mrp_posterior_pairs_free(&match);
    mrp_posterior_pairs_free(&gap_x);
    mrp_posterior_pairs_free(&gap_y);
    mrp_context_destroy(ctx);
    return 0;
}
