/*
 * phase_from_alignments_downsampled.c -- margin phase's whole chunk loop (phase.c:337-436) from plain C, in one device call, the
 * downsampling to polish.maxDepth (phase.c:360-382) included:
 *
 *   mrp_context_set_downsampling(ctx, max_depth, seed)
 *   alignments + VCF entries + filtered VCF entries --mrp_phase_aligned_chunks_with_filtered (keep = NULL)-->
 *       haplotypes, HP tags of the primary reads, the filtered variants phased, the filtered reads -- the discards among them -- tagged
 *
 * The mask is made on the device from the extraction's per-read state and never comes from the caller.  For comparison the example
 * also makes it the long way round, as a caller who chains the single calls would: mrp_extract_read_substrings,
 * mrp_aln_read_lengths, mrp_downsample_keep_from_extracted -- the definition the one call is held to.  The input is one small
 * hand-made chunk: a 40-base reference slice at genome 100, two primary variants, two filtered ones, a dozen reads whose bases cycle
 * A C G T; nine of them are kept and cover both variants, and with max_depth 6 the three shortest are discarded.  Prints the input (so that a caller in another language
 * can rebuild it), the state machines, the mask and the probabilities of the long way round, and every result, doubles as hexadecimal.
 *
 *   gcc -O2 -Iinclude examples/phase_from_alignments_downsampled.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o phase_from_alignments_downsampled
 */
#include <math.h>
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

enum { N_VARIANTS = 2, N_ALLELES = 5, N_FVARIANTS = 2, N_FALLELES = 4, N_READS = 12, MAX_OPS = 8 };

static const char REFERENCE[] = "ACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAAC"; /* genome 100..139 */
static const int64_t VARIANT_POS[N_VARIANTS] = {110, 118};
static const int64_t ALLELE_FIRST[N_VARIANTS + 1] = {0, 2, 5};
static const char *ALLELES[N_ALLELES] = {"A", "G", "A", "T", "ACG"}; /* allele 0 of a variant = REF */
static const int64_t FVARIANT_POS[N_FVARIANTS] = {125, 131}; /* the filtered VCF entries of the chunk */
static const int64_t FALLELE_FIRST[N_FVARIANTS + 1] = {0, 2, 4};
static const char *FALLELES[N_FALLELES] = {"G", "C", "C", "T"};
static const int32_t FGENOTYPE[2 * N_FVARIANTS] = {0, 1, 1, 0};
static const struct { int64_t pos; const char *cigar; uint8_t mapq; uint16_t flag; } READS[N_READS] = {
    {100, "30M", 60, 0},    {100, "30M", 60, 0x10}, {101, "29M", 60, 0},    {105, "3S25M", 60, 0x10}, {102, "12M2I14M", 60, 0},
    {104, "8M3D15M", 60, 0x10}, {100, "40M", 3, 0}, {103, "27M", 60, 0},    {103, "37M", 60, 0x10},   {120, "15M", 60, 0},
    {100, "16M1I12M", 60, 0},   {100, "30M", 60, 0x100},
};
static const int64_t MAX_DEPTH = 6; /* polish.maxDepth: 32 or 64 in the shipped parameter files; 6 for a dozen reads */
static const uint64_t SEED = 7;

static int parse_cigar(const char *text, uint32_t *words, int32_t *query_len) {
    static const char OPS[] = "MIDNSHP=X";
    int n = 0;
    *query_len = 0;
    for (const char *p = text; *p;) {
        uint32_t len = 0;
        while (*p >= '0' && *p <= '9') len = 10 * len + (uint32_t) (*p++ - '0');
        const uint32_t op = (uint32_t) (strchr(OPS, *p++) - OPS);
        words[n++] = len << 4 | op;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) *query_len += (int32_t) len;
    }
    return n;
}

static int64_t pack_alleles(const char *const *alleles, int n, char *chars, int64_t *off, int32_t *len) {
    int64_t at = 0;
    for (int a = 0; a < n; a++) {
        off[a] = at;
        len[a] = (int32_t) strlen(alleles[a]);
        memcpy(chars + at, alleles[a], (size_t) len[a]);
        at += len[a];
    }
    return at;
}

static void print_doubles(const char *name, const double *v, int64_t n) {
    printf("%s", name);
    for (int64_t i = 0; i < n; i++) printf(" %a", v[i]);
    printf("\n");
}

int main(void) {
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

    /* the chunk as htslib holds it: alleles as chars in one buffer, CIGARs as BAM words, bases as 4-bit codes (A C G T = 1 2 4 8) */
    char allele_chars[64], fallele_chars[64];
    int64_t allele_off[N_ALLELES], fallele_off[N_FALLELES];
    int32_t allele_len[N_ALLELES], fallele_len[N_FALLELES];
    const int64_t allele_bytes = pack_alleles(ALLELES, N_ALLELES, allele_chars, allele_off, allele_len);
    const int64_t fallele_bytes = pack_alleles(FALLELES, N_FALLELES, fallele_chars, fallele_off, fallele_len);
    const uint8_t is_sv[N_VARIANTS] = {0, 0}, fis_sv[N_FVARIANTS] = {0, 0};
    int64_t pos[N_READS], cigar_first[N_READS + 1] = {0}, seq_first[N_READS + 1] = {0};
    uint16_t flag[N_READS];
    uint8_t mapq[N_READS], seq[N_READS * 32];
    int32_t l_qseq[N_READS];
    uint32_t cigar[N_READS * MAX_OPS];
    char names[N_READS][16];
    const char *name_ptr[N_READS];
    memset(seq, 0, sizeof(seq));
    for (int r = 0; r < N_READS; r++) {
        pos[r] = READS[r].pos;
        flag[r] = READS[r].flag;
        mapq[r] = READS[r].mapq;
        snprintf(names[r], sizeof(names[r]), "hand%d", r);
        name_ptr[r] = names[r];
        cigar_first[r + 1] = cigar_first[r] + parse_cigar(READS[r].cigar, cigar + cigar_first[r], &l_qseq[r]);
        for (int i = 0; i < l_qseq[r]; i++) seq[seq_first[r] + i / 2] |= (uint8_t) ((1 << (i % 4)) << (i % 2 ? 0 : 4)); /* high nibble first */
        seq_first[r + 1] = seq_first[r] + (l_qseq[r] + 1) / 2;
    }
    mrp_aligned_chunk chunk;
    memset(&chunk, 0, sizeof(chunk));
    chunk.overlap_start = chunk.chunk_start = 100;
    chunk.overlap_end = chunk.chunk_end = 140;
    chunk.reference = REFERENCE;
    chunk.reference_len = 40;
    chunk.n_variants = N_VARIANTS;
    chunk.variant_pos = VARIANT_POS;
    chunk.allele_first = ALLELE_FIRST;
    chunk.allele_off = allele_off;
    chunk.allele_len = allele_len;
    chunk.allele_chars = allele_chars;
    chunk.allele_bytes = allele_bytes;
    chunk.is_sv = is_sv;
    chunk.n_reads = N_READS;
    chunk.pos = pos;
    chunk.flag = flag;
    chunk.mapq = mapq;
    chunk.l_qseq = l_qseq;
    chunk.cigar_first = cigar_first;
    chunk.cigar = cigar;
    chunk.seq_first = seq_first;
    chunk.seq = seq;
    mrp_aligned_chunk_rest rest;
    memset(&rest, 0, sizeof(rest));
    rest.n_variants = N_FVARIANTS;
    rest.variant_pos = FVARIANT_POS;
    rest.allele_first = FALLELE_FIRST;
    rest.allele_off = fallele_off;
    rest.allele_len = fallele_len;
    rest.allele_chars = fallele_chars;
    rest.allele_bytes = fallele_bytes;
    rest.is_sv = fis_sv;
    rest.gt = FGENOTYPE;

    /* small windows, as the reference slice is small; everything else as shipped.  min_phred 30 leaves primary reads untagged: they are
     * tagged with the filtered ones */
    const mrp_extract_options options = {2, 6, 5, 0, 0, 0, 0};
    mrp_params params = {1, 1, 1, 0, 100, 100, 0.0, 64, 2, 10}; /* params/base_params.json "phase" */
    const char *const *read_names[1] = {name_ptr};
    int8_t hap[N_READS];
    double phred[N_READS];
    int8_t *hap_out[1] = {hap};
    double *phred_out[1] = {phred};
    mrp_phase_result *res[1] = {NULL};
    int64_t *bubble_variant[1] = {NULL};
    mrp_filtered_out out;
    int32_t *filtered_read[1] = {NULL};
    mrp_phase_aligned_filtered_stats st;
    /* the one call: the setting on, no mask from the caller (a mask would now be MRP_ERR_ARG) */
    CHECK(mrp_context_set_downsampling(ctx, MAX_DEPTH, SEED));
    CHECK(mrp_phase_aligned_chunks_with_filtered(ctx, 1, &chunk, &rest, read_names, NULL, &options, &fwd, &rev, 4, 512, 0.0, &params, 30, res, hap_out,
                                                 phred_out, NULL, bubble_variant, &out, filtered_read, &st));
    mrp_downsampling_stats ds;
    CHECK(mrp_context_last_downsampling(ctx, &ds));

    /* the long way round: the chunk's primary extraction, h from the CIGARs, the definition on the host */
    mrp_extracted_chunk *x = NULL;
    int32_t aln_len[N_READS], downsampled = 0;
    uint8_t keep[N_READS];
    double prob[N_READS];
    CHECK(mrp_extract_read_substrings(ctx, 1, &chunk, &options, &x, NULL));
    CHECK(mrp_aln_read_lengths(&chunk, aln_len));
    CHECK(mrp_downsample_keep_from_extracted(&x[0], aln_len, MAX_DEPTH, SEED, chunk.overlap_start, chunk.overlap_end, keep, prob, &downsampled));

    for (int v = 0; v < N_VARIANTS; v++) {
        printf("variant %lld", (long long) VARIANT_POS[v]);
        for (int64_t a = ALLELE_FIRST[v]; a < ALLELE_FIRST[v + 1]; a++) printf(" %s", ALLELES[a]);
        printf("\n");
    }
    for (int v = 0; v < N_FVARIANTS; v++) {
        printf("fvariant %lld %d %d", (long long) FVARIANT_POS[v], FGENOTYPE[2 * v], FGENOTYPE[2 * v + 1]);
        for (int64_t a = FALLELE_FIRST[v]; a < FALLELE_FIRST[v + 1]; a++) printf(" %s", FALLELES[a]);
        printf("\n");
    }
    for (int r = 0; r < N_READS; r++)
        printf("read %lld %s %d %d\n", (long long) READS[r].pos, READS[r].cigar, READS[r].mapq, READS[r].flag);
    printf("downsampling %lld %llu %d\n", (long long) MAX_DEPTH, (unsigned long long) SEED, downsampled);
    printf("status");
    for (int r = 0; r < N_READS; r++) printf(" %d", x[0].read_status[r]);
    printf("\nn_substrings");
    for (int r = 0; r < N_READS; r++) printf(" %d", x[0].read_n_substrings[r]);
    printf("\naln_len");
    for (int r = 0; r < N_READS; r++) printf(" %d", aln_len[r]);
    printf("\nkeep");
    for (int r = 0; r < N_READS; r++) printf(" %d", keep[r]);
    printf("\n");
    print_doubles("prob", prob, N_READS);
    print_doubles("model_f", &fwd.match_continue, (int64_t) (sizeof(fwd) / sizeof(double)));
    print_doubles("model_r", &rev.match_continue, (int64_t) (sizeof(rev) / sizeof(double)));
    printf("hap");
    for (int r = 0; r < N_READS; r++) printf(" %d", hap[r]);
    printf("\nbubble_variant");
    for (int64_t b = 0; bubble_variant[0][b] != -1; b++) printf(" %lld", (long long) bubble_variant[0][b]);
    printf("\nfiltered_read");
    int64_t n_filtered = 0;
    for (; filtered_read[0][n_filtered] != -1; n_filtered++) printf(" %d", filtered_read[0][n_filtered]);
    printf("\nread_hap");
    for (int64_t r = 0; r < out.n_reads; r++) printf(" %d", out.read_hap[r]);
    printf("\nvariant_state");
    for (int64_t v = 0; v < out.n_variants; v++) printf(" %d", out.variant_state[v]);
    printf("\n");
    print_doubles("phred", phred, N_READS);
    print_doubles("h1", out.h1, out.n_reads);
    print_doubles("h2", out.h2, out.n_reads);
    print_doubles("cis", out.cis, out.n_variants);
    print_doubles("trans", out.trans, out.n_variants);
    int64_t tagged = 0;
    for (int64_t f = 0; f < n_filtered; f++) tagged += out.read_hap[N_READS + f] > 0;
    printf("discarded %lld of_chunks %lld downsampled %lld mask_bytes %lld\n", (long long) ds.reads_discarded, (long long) ds.chunks,
           (long long) ds.chunks_downsampled, (long long) ds.bytes_downloaded);
    printf("%s: %lld pairs in one launch, resident=%d; the downsampling kernel took %.3f ms and discarded %lld reads; %lld filtered variants phased, "
           "%lld of %lld filtered reads tagged; %lld bytes downloaded before the launch\n",
           mrp_version(), (long long) st.pairs_scored, st.aligned.chunks.phase.resident, ds.downsample_ms, (long long) ds.reads_discarded,
           (long long) st.filtered_variants, (long long) tagged, (long long) n_filtered, (long long) st.aligned.front_bytes_downloaded);
    {
        void *arrays[] = {x[0].ref_aln_start, x[0].ref_aln_stop_incl, x[0].allele_first, x[0].allele_off, x[0].allele_len, x[0].read_status,
                          x[0].read_n_substrings, x[0].entry_first, x[0].entry_read, x[0].entry_off, x[0].entry_len, x[0].pool};
        for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); i++) mrp_free(arrays[i]);
        mrp_free(x);
    }
    mrp_phase_result_destroy(res[0]);
    mrp_free(bubble_variant[0]);
    mrp_free(filtered_read[0]);
    mrp_free(out.read_hap); mrp_free(out.h1); mrp_free(out.h2); mrp_free(out.variant_state); mrp_free(out.cis); mrp_free(out.trans);
    mrp_context_destroy(ctx);
    return 0;
}
