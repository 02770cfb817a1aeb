/*
 * phase_from_alignments_records.c -- from alignments to a phased VCF's phase sets, from plain C:
 *
 *   alignments + VCF entries + filtered VCF entries --mrp_phase_aligned_chunks_with_records-->
 *       haplotypes, HP tags, the filtered variants phased, and per variant what writePhasedVcf reads (the phased variant records)
 *   --mrp_stitch_chunk--> which chunks trade their haplotypes   --mrp_variants_from_records--> the contig's updated variants
 *   --mrp_phase_sets--> their phase sets
 *
 * The input is one small hand-made reference slice at genome 100 cut into two adjacent chunks, [100, 120) and [120, 140), that see the
 * same dozen reads (their overlap is the whole slice): two primary variants, two filtered ones, reads whose bases cycle A C G T, one of
 * them taken out by the caller's downsampling mask.  Prints the input, the state machines, every record and the phase sets.
 *
 *   gcc -O2 -Iinclude examples/phase_from_alignments_records.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o phase_from_alignments_records
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

enum { N_CHUNKS = 2, N_VARIANTS = 2, N_ALLELES = 5, N_FVARIANTS = 2, N_FALLELES = 4, N_READS = 12, MAX_OPS = 8 };

static const char REFERENCE[] = "ACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAAC"; /* genome 100..139 */
static const int64_t VARIANT_POS[N_VARIANTS] = {110, 118};
static const int64_t ALLELE_FIRST[N_VARIANTS + 1] = {0, 2, 5};
static const char *ALLELES[N_ALLELES] = {"A", "G", "A", "T", "ACG"}; /* allele 0 of a variant = REF */
static const int64_t FVARIANT_POS[N_FVARIANTS] = {125, 131}; /* the filtered VCF entries of the chunk */
static const int64_t FALLELE_FIRST[N_FVARIANTS + 1] = {0, 2, 4};
static const char *FALLELES[N_FALLELES] = {"G", "C", "C", "T"};
static const int32_t FGENOTYPE[2 * N_FVARIANTS] = {0, 1, 1, 0};
static const struct { int64_t pos; const char *cigar; uint8_t mapq; uint16_t flag; uint8_t keep; } READS[N_READS] = {
    {100, "30M", 60, 0, 1},    {100, "30M", 60, 0x10, 1}, {101, "29M", 60, 0, 1},    {105, "3S25M", 60, 0x10, 1}, {102, "12M2I14M", 60, 0, 1},
    {104, "8M3D15M", 60, 0x10, 1}, {100, "40M", 3, 0, 1}, {103, "27M", 60, 0, 0},    {103, "37M", 60, 0x10, 1},   {120, "15M", 60, 0, 1},
    {100, "16M1I12M", 60, 0, 1},   {100, "30M", 60, 0x100, 1},
};

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
    uint8_t mapq[N_READS], keep[N_READS], seq[N_READS * 32];
    int32_t l_qseq[N_READS];
    uint32_t cigar[N_READS * MAX_OPS];
    char names[N_READS][16];
    const char *name_ptr[N_READS];
    memset(seq, 0, sizeof(seq));
    for (int r = 0; r < N_READS; r++) {
        pos[r] = READS[r].pos;
        flag[r] = READS[r].flag;
        mapq[r] = READS[r].mapq;
        keep[r] = READS[r].keep;
        snprintf(names[r], sizeof(names[r]), "hand%d", r);
        name_ptr[r] = names[r];
        cigar_first[r + 1] = cigar_first[r] + parse_cigar(READS[r].cigar, cigar + cigar_first[r], &l_qseq[r]);
        for (int i = 0; i < l_qseq[r]; i++) seq[seq_first[r] + i / 2] |= (uint8_t) ((1 << (i % 4)) << (i % 2 ? 0 : 4)); /* high nibble first */
        seq_first[r + 1] = seq_first[r] + (l_qseq[r] + 1) / 2;
    }
    mrp_aligned_chunk chunk;
    memset(&chunk, 0, sizeof(chunk));
    chunk.overlap_start = chunk.chunk_start = 100;
    chunk.overlap_end = 140;
    chunk.chunk_end = 120;
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

    /* two adjacent chunks over the one slice: [100, 120) and [120, 140) */
    mrp_aligned_chunk chunks[N_CHUNKS] = {chunk, chunk};
    chunks[1].chunk_start = 120;
    chunks[1].chunk_end = 140;
    const mrp_aligned_chunk_rest rests[N_CHUNKS] = {rest, rest};

    /* small windows, as the reference slice is small; everything else as shipped.  min_phred 0: every read the phasing put into a
     * partition keeps its tag (over two sites the scores stay small), and only tagged reads are listed under an allele */
    const mrp_extract_options options = {2, 6, 5, 0, 0, 0, 0};
    mrp_params params = {1, 1, 1, 0, 100, 100, 0.0, 64, 2, 10}; /* params/base_params.json "phase" */
    const char *const *read_names[N_CHUNKS] = {name_ptr, name_ptr};
    const uint8_t *keeps[N_CHUNKS] = {keep, keep};
    int8_t hap[N_CHUNKS][N_READS];
    int8_t *hap_out[N_CHUNKS] = {hap[0], hap[1]};
    mrp_phase_result *res[N_CHUNKS] = {NULL, NULL};
    int64_t *bubble_variant[N_CHUNKS] = {NULL, NULL};
    mrp_filtered_out out[N_CHUNKS];
    int32_t *filtered_read[N_CHUNKS] = {NULL, NULL};
    mrp_variant_records records[N_CHUNKS];
    mrp_phase_aligned_records_stats st;
    CHECK(mrp_phase_aligned_chunks_with_records(ctx, N_CHUNKS, chunks, rests, read_names, keeps, &options, &fwd, &rev, 4, 512, 0.0, &params, 0, res, hap_out,
                                                NULL, NULL, bubble_variant, out, filtered_read, records, &st));

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
        printf("read %lld %s %d %d %d\n", (long long) READS[r].pos, READS[r].cigar, READS[r].mapq, READS[r].flag, READS[r].keep);
    print_doubles("model_f", &fwd.match_continue, (int64_t) (sizeof(fwd) / sizeof(double)));
    print_doubles("model_r", &rev.match_continue, (int64_t) (sizeof(rev) / sizeof(double)));

    /* the records: per site its state, genotype, log probabilities (writePhasedVcf applies toPhred(exp(.))) and the two read lists */
    for (int c = 0; c < N_CHUNKS; c++) {
        const mrp_variant_records *R = &records[c];
        for (int64_t s = 0; s < R->n_primary + R->n_filtered; s++) {
            printf("record %d %lld %d %d %d %a %a %a %d %d", c, (long long) s, R->state[s], R->gt[2 * s], R->gt[2 * s + 1], (double) R->genotype_log_prob[s],
                   (double) R->hap1_log_prob[s], (double) R->hap2_log_prob[s], R->n_hap1[s], R->n_hap2[s]);
            for (int64_t k = R->read_first[s]; k < R->read_first[s + 1]; k++) printf(" %d", R->reads[k]);
            printf("\n");
        }
    }

    /* stitching (stitching.c:345-403) over the reads each chunk tagged, the first chunk never switched */
    mrp_stitch *stitch = NULL;
    CHECK(mrp_stitch_create(&stitch));
    int32_t switched[N_CHUNKS];
    for (int c = 0; c < N_CHUNKS; c++) {
        const char *n1[N_READS], *n2[N_READS];
        double p1[N_READS], p2[N_READS];
        int64_t k1 = 0, k2 = 0;
        for (int r = 0; r < N_READS; r++) {
            if (out[c].read_hap[r] == 1) { n1[k1] = names[r]; p1[k1++] = 1.0; }
            if (out[c].read_hap[r] == 2) { n2[k2] = names[r]; p2[k2++] = 1.0; }
        }
        int sw = 0;
        CHECK(mrp_stitch_chunk(stitch, k1, n1, p1, k2, n2, p2, 0, c == 0, &sw, NULL));
        switched[c] = sw;
    }
    printf("switched %d %d\n", switched[0], switched[1]);

    /* the contig's updated variants, read ids = read indices here (both chunks hold the same reads), and their phase sets */
    int32_t read_id[N_READS], n_alleles[N_VARIANTS], fn_alleles[N_FVARIANTS];
    for (int r = 0; r < N_READS; r++) read_id[r] = r;
    for (int v = 0; v < N_VARIANTS; v++) n_alleles[v] = (int32_t) (ALLELE_FIRST[v + 1] - ALLELE_FIRST[v]);
    for (int v = 0; v < N_FVARIANTS; v++) fn_alleles[v] = (int32_t) (FALLELE_FIRST[v + 1] - FALLELE_FIRST[v]);
    const int64_t *vpos[N_CHUNKS] = {VARIANT_POS, VARIANT_POS}, *fpos[N_CHUNKS] = {FVARIANT_POS, FVARIANT_POS};
    const int32_t *na[N_CHUNKS] = {n_alleles, n_alleles}, *fna[N_CHUNKS] = {fn_alleles, fn_alleles}, *ids[N_CHUNKS] = {read_id, read_id};
    mrp_record_variants vars;
    CHECK(mrp_variants_from_records(N_CHUNKS, records, vpos, na, fpos, fna, switched, ids, &vars));
    int32_t phase_set[N_CHUNKS * (N_VARIANTS + N_FVARIANTS)], reason[N_CHUNKS * (N_VARIANTS + N_FVARIANTS)];
    CHECK(mrp_phase_sets(vars.n_variants, vars.variants, 2, 0.05, 0.5, phase_set, reason)); /* phasesetMinSpanningReads, ...MinBinomialReadSplitLikelihood, ...MaxDiscordantRatio */
    for (int64_t i = 0; i < vars.n_variants; i++)
        printf("phased %d %d|%d chunk %d site %d PS %d reason %d\n", vars.variants[i].pos, vars.variants[i].gt1, vars.variants[i].gt2, vars.chunk[i], vars.site[i],
               phase_set[i], reason[i]);
    printf("%s: %lld sites, %lld updated, %lld reads listed; %lld bytes of records downloaded; records kernel %.3f ms beside %.3f ms of the back half\n",
           mrp_version(), (long long) st.records_sites, (long long) st.records_updated, (long long) st.reads_listed, (long long) st.records_bytes_downloaded,
           st.records_ms, st.filtered.filtered_ms);

    mrp_free(vars.variants);
    mrp_stitch_destroy(stitch);
    for (int c = 0; c < N_CHUNKS; c++) {
        mrp_variant_records *R = &records[c];
        mrp_free(R->state); mrp_free(R->gt); mrp_free(R->genotype_log_prob); mrp_free(R->hap1_log_prob); mrp_free(R->hap2_log_prob);
        mrp_free(R->read_first); mrp_free(R->n_hap1); mrp_free(R->n_hap2); mrp_free(R->reads);
        mrp_phase_result_destroy(res[c]);
        mrp_free(bubble_variant[c]);
        mrp_free(filtered_read[c]);
        mrp_free(out[c].read_hap); mrp_free(out[c].h1); mrp_free(out[c].h2); mrp_free(out[c].variant_state); mrp_free(out[c].cis); mrp_free(out[c].trans);
    }
    mrp_context_destroy(ctx);
    return 0;
}
