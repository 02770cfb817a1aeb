/*
 * phase_contig_queue.c -- a contig from alignments to phase sets and final HP tags through the work queue, from plain C:
 *
 *   alignments + VCF entries + filtered VCF entries of a contig's chunks --mrp_queue_phase_aligned_chunks_with_records-->
 *       per chunk its haplotypes, HP tags and scores, the filtered variants phased, the filtered reads tagged and the phased variant
 *       records, whichever lane of whichever device phased it
 *   --mrp_close_contig--> which chunks trade their haplotypes, the contig's updated variants with their phase sets, and the final
 *       HP tag of every read (what margin phase does after its chunk loop, phase.c:475-535)
 *
 * The input is one small hand-made reference slice at genome 100 cut into three adjacent chunks, [100, 114), [114, 127) and [127, 140),
 * that see the same dozen reads (their overlap is the whole slice): two primary variants, two filtered ones, reads whose bases cycle
 * A C G T, one of them taken out by the caller's downsampling mask.  Prints the input, the state machines, the switches, the phased
 * variants and the tags.
 *
 *   gcc -O2 -Iinclude examples/phase_contig_queue.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o phase_contig_queue
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

enum { N_CHUNKS = 3, N_VARIANTS = 2, N_ALLELES = 5, N_FVARIANTS = 2, N_FALLELES = 4, N_READS = 12, MAX_OPS = 8 };

static const char REFERENCE[] = "ACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAAC"; /* genome 100..139 */
static const int64_t CHUNK_START[N_CHUNKS] = {100, 114, 127}, CHUNK_END[N_CHUNKS] = {114, 127, 140};
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
    /* one queue over device 0; a node's worth of devices is listed the same way */
    const int32_t devices[1] = {0};
    mrp_queue *queue = NULL;
    CHECK(mrp_queue_create(devices, 1, &queue));

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
    int32_t l_qseq[N_READS], read_id[N_READS];
    uint32_t cigar[N_READS * MAX_OPS];
    char names[N_READS][16];
    const char *name_ptr[N_READS];
    memset(seq, 0, sizeof(seq));
    for (int r = 0; r < N_READS; r++) {
        pos[r] = READS[r].pos;
        flag[r] = READS[r].flag;
        mapq[r] = READS[r].mapq;
        keep[r] = READS[r].keep;
        read_id[r] = r; /* the caller's global read ids: every chunk holds the same reads here */
        snprintf(names[r], sizeof(names[r]), "hand%d", r);
        name_ptr[r] = names[r];
        cigar_first[r + 1] = cigar_first[r] + parse_cigar(READS[r].cigar, cigar + cigar_first[r], &l_qseq[r]);
        for (int i = 0; i < l_qseq[r]; i++) seq[seq_first[r] + i / 2] |= (uint8_t) ((1 << (i % 4)) << (i % 2 ? 0 : 4)); /* high nibble first */
        seq_first[r + 1] = seq_first[r] + (l_qseq[r] + 1) / 2;
    }
    mrp_aligned_chunk chunk;
    memset(&chunk, 0, sizeof(chunk));
    chunk.overlap_start = 100;
    chunk.overlap_end = 140;
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

    /* three adjacent chunks over the one slice, in genome order */
    mrp_aligned_chunk chunks[N_CHUNKS];
    mrp_aligned_chunk_rest rests[N_CHUNKS];
    for (int c = 0; c < N_CHUNKS; c++) {
        chunks[c] = chunk;
        chunks[c].chunk_start = CHUNK_START[c];
        chunks[c].chunk_end = CHUNK_END[c];
        rests[c] = rest;
    }

    /* small windows, as the reference slice is small; everything else as shipped.  min_phred 0: every read the phasing put into a
     * partition keeps its tag (over two sites the scores stay small).  One chunk per batch: the three chunks go through the queue's
     * lanes as three calls, and every output lands at its chunk's own position */
    const mrp_extract_options options = {2, 6, 5, 0, 0, 0, 0};
    mrp_params params = {1, 1, 1, 0, 100, 100, 0.0, 64, 2, 10}; /* params/base_params.json "phase" */
    const char *const *read_names[N_CHUNKS] = {name_ptr, name_ptr, name_ptr};
    const uint8_t *keeps[N_CHUNKS] = {keep, keep, keep};
    int8_t hap[N_CHUNKS][N_READS];
    double phred[N_CHUNKS][N_READS];
    int8_t *hap_out[N_CHUNKS] = {hap[0], hap[1], hap[2]};
    double *phred_out[N_CHUNKS] = {phred[0], phred[1], phred[2]};
    mrp_phase_result *res[N_CHUNKS] = {NULL, NULL, NULL};
    int64_t *bubble_variant[N_CHUNKS] = {NULL, NULL, NULL};
    mrp_filtered_out out[N_CHUNKS];
    int32_t *filtered_read[N_CHUNKS] = {NULL, NULL, NULL};
    mrp_variant_records records[N_CHUNKS];
    mrp_queue_stats st;
    mrp_queue_records_stats rst;
    CHECK(mrp_queue_phase_aligned_chunks_with_records(queue, N_CHUNKS, chunks, rests, read_names, keeps, &options, &fwd, &rev, 4, 512, 0.0, &params, 0, 1, res,
                                                      hap_out, phred_out, NULL, bubble_variant, out, filtered_read, records, &st, &rst));

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
    for (int c = 0; c < N_CHUNKS; c++) printf("chunk %lld %lld\n", (long long) CHUNK_START[c], (long long) CHUNK_END[c]);
    print_doubles("model_f", &fwd.match_continue, (int64_t) (sizeof(fwd) / sizeof(double)));
    print_doubles("model_r", &rev.match_continue, (int64_t) (sizeof(rev) / sizeof(double)));

    /* closing the contig: the library derives every read's final tag and the value it carries into the stitching, stitches chunk by
     * chunk, applies the switches to the records and runs writePhasedVcf's phase set rules */
    int32_t n_alleles[N_VARIANTS], fn_alleles[N_FVARIANTS];
    for (int v = 0; v < N_VARIANTS; v++) n_alleles[v] = (int32_t) (ALLELE_FIRST[v + 1] - ALLELE_FIRST[v]);
    for (int v = 0; v < N_FVARIANTS; v++) fn_alleles[v] = (int32_t) (FALLELE_FIRST[v + 1] - FALLELE_FIRST[v]);
    mrp_contig_chunk cc[N_CHUNKS];
    memset(cc, 0, sizeof(cc));
    for (int c = 0; c < N_CHUNKS; c++) {
        cc[c].n_reads = N_READS;
        cc[c].read_names = name_ptr;
        cc[c].read_id = read_id;
        cc[c].hap_out = hap[c];
        cc[c].phred_out = phred[c];
        cc[c].filtered_out = &out[c];
        cc[c].filtered_read_out = filtered_read[c];
        cc[c].records = &records[c];
        cc[c].n_variants = N_VARIANTS;
        cc[c].n_fvariants = N_FVARIANTS;
        cc[c].variant_pos = VARIANT_POS;
        cc[c].n_alleles = n_alleles;
        cc[c].fvariant_pos = FVARIANT_POS;
        cc[c].fn_alleles = fn_alleles;
    }
    /* stitchWithPrimaryReadsOnly off, switching allowed; phasesetMinSpanningReads, ...MinBinomialReadSplitLikelihood, ...MaxDiscordantRatio */
    const mrp_contig_rules rules = {0, 0, 2, 0.05, 0.5};
    mrp_contig_out closed;
    CHECK(mrp_close_contig(N_CHUNKS, cc, &rules, &closed));

    for (int c = 0; c < N_CHUNKS; c++)
        printf("stitched %d switched %d counts %lld %lld %lld %lld\n", c, closed.switched[c], (long long) closed.counts[4 * c], (long long) closed.counts[4 * c + 1],
               (long long) closed.counts[4 * c + 2], (long long) closed.counts[4 * c + 3]);
    for (int64_t i = 0; i < closed.variants.n_variants; i++)
        printf("phased %d %d|%d chunk %d site %d PS %d reason %d\n", closed.variants.variants[i].pos, closed.variants.variants[i].gt1, closed.variants.variants[i].gt2,
               closed.variants.chunk[i], closed.variants.site[i], closed.phase_set[i], closed.reason[i]);
    for (int c = 0; c < N_CHUNKS; c++) {
        printf("tags %d", c);
        for (int r = 0; r < N_READS; r++) printf(" %d", closed.final_hap[c][r]);
        printf("\n");
    }
    printf("%s: %lld batches; %lld sites, %lld updated, %lld reads listed; %lld bytes of records downloaded\n", mrp_version(), (long long) st.batches,
           (long long) rst.records_sites, (long long) rst.records_updated, (long long) rst.reads_listed, (long long) rst.records_bytes_downloaded);

    mrp_contig_out_clear(&closed);
    for (int c = 0; c < N_CHUNKS; c++) {
        mrp_variant_records *R = &records[c];
        mrp_free(R->state); mrp_free(R->gt); mrp_free(R->genotype_log_prob); mrp_free(R->hap1_log_prob); mrp_free(R->hap2_log_prob);
        mrp_free(R->read_first); mrp_free(R->n_hap1); mrp_free(R->n_hap2); mrp_free(R->reads);
        mrp_phase_result_destroy(res[c]);
        mrp_free(bubble_variant[c]);
        mrp_free(filtered_read[c]);
        mrp_free(out[c].read_hap); mrp_free(out[c].h1); mrp_free(out[c].h2); mrp_free(out[c].variant_state); mrp_free(out[c].cis); mrp_free(out[c].trans);
    }
    mrp_queue_destroy(queue);
    return 0;
}
