/*
 * haplotag_from_alignments_queue.c -- the chunk loop of tools/tagFromPhasedVcf.c (:227-309) from plain C, over the work queue:
 *
 *   n x (alignments + phased VCF entries) --mrp_haplotag_aligned_chunks_on_devices--> per chunk: haplotype tag per read
 *
 * The input is the hand-made chunk of haplotag_from_alignments.c, three times, on device 0, one chunk per batch: the queue orders the
 * chunks by mrp_haplotag_chunk_units, hands the batches to its lanes and writes every chunk's results at the chunk's own position -- bit
 * for bit what the one call gives.  Prints the input once, the state machines, and for every copy what that example prints, doubles as
 * hexadecimal; then one line of the queue's stats.
 *
 *   gcc -O2 -Iinclude examples/haplotag_from_alignments_queue.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o haplotag_from_alignments_queue
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

enum { N_COPIES = 3, N_VARIANTS = 3, N_ALLELES = 7, N_READS = 12, MAX_OPS = 8 };

static const char REFERENCE[] = "ACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAAC"; /* genome 100..139 */
static const int64_t VARIANT_POS[N_VARIANTS] = {110, 118, 125};
static const int64_t ALLELE_FIRST[N_VARIANTS + 1] = {0, 2, 5, 7};
static const char *ALLELES[N_ALLELES] = {"A", "G", "A", "T", "ACG", "G", "C"}; /* allele 0 of a variant = REF */
static const int32_t GENOTYPE[2 * N_VARIANTS] = {0, 1, 2, 0, 1, 1}; /* gt1 | gt2 of the phased VCF; the last one is homozygous */
static const struct { int64_t pos; const char *cigar; uint8_t mapq; uint16_t flag; } READS[N_READS] = {
    {100, "30M", 60, 0},      {100, "30M", 60, 0x10},  {101, "29M", 60, 0},     {105, "3S25M", 60, 0x10}, {102, "12M2I14M", 60, 0}, {104, "8M3D15M", 60, 0x10},
    {100, "40M", 3, 0},       {103, "27M", 60, 0},     {103, "27M", 60, 0x10},  {120, "15M", 60, 0},      {100, "16M1I12M", 60, 0}, {100, "30M", 60, 0x100},
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

static void print_doubles(const char *name, const double *v, int n) {
    printf("%s", name);
    for (int i = 0; i < n; i++) printf(" %a", v[i]);
    printf("\n");
}

int main(void) {
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
    char allele_chars[64];
    int64_t allele_off[N_ALLELES];
    int32_t allele_len[N_ALLELES];
    int64_t at = 0;
    for (int a = 0; a < N_ALLELES; a++) {
        allele_off[a] = at;
        allele_len[a] = (int32_t) strlen(ALLELES[a]);
        memcpy(allele_chars + at, ALLELES[a], (size_t) allele_len[a]);
        at += allele_len[a];
    }
    const uint8_t is_sv[N_VARIANTS] = {0, 0, 0};
    int64_t pos[N_READS], cigar_first[N_READS + 1] = {0}, seq_first[N_READS + 1] = {0};
    uint16_t flag[N_READS];
    uint8_t mapq[N_READS], seq[N_READS * 32];
    int32_t l_qseq[N_READS];
    uint32_t cigar[N_READS * MAX_OPS];
    memset(seq, 0, sizeof(seq));
    for (int r = 0; r < N_READS; r++) {
        pos[r] = READS[r].pos;
        flag[r] = READS[r].flag;
        mapq[r] = READS[r].mapq;
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
    chunk.allele_bytes = at;
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

    /* small windows, as the reference slice is small; everything else as shipped */
    const mrp_extract_options options = {2, 6, 5, 0, 0, 0, 0};
    mrp_aligned_chunk chunks[N_COPIES];
    const int32_t *gt[N_COPIES];
    int8_t hap[N_COPIES][N_READS];
    double h1[N_COPIES][N_READS], h2[N_COPIES][N_READS];
    int8_t *hap_out[N_COPIES];
    double *h1_out[N_COPIES], *h2_out[N_COPIES];
    for (int c = 0; c < N_COPIES; c++) {
        chunks[c] = chunk;
        gt[c] = GENOTYPE;
        hap_out[c] = hap[c];
        h1_out[c] = h1[c];
        h2_out[c] = h2[c];
    }
    int64_t units = 0;
    CHECK(mrp_haplotag_chunk_units(&chunk, GENOTYPE, &units));
    const int32_t devices[1] = {0};
    mrp_queue_stats st;
    CHECK(mrp_haplotag_aligned_chunks_on_devices(devices, 1, N_COPIES, chunks, gt, &options, &fwd, &rev, 4, 1 /* chunk per batch */, hap_out, h1_out,
                                                 h2_out, &st));

    for (int v = 0; v < N_VARIANTS; v++) {
        printf("variant %lld %d %d", (long long) VARIANT_POS[v], GENOTYPE[2 * v], GENOTYPE[2 * v + 1]);
        for (int64_t a = ALLELE_FIRST[v]; a < ALLELE_FIRST[v + 1]; a++) printf(" %s", ALLELES[a]);
        printf("\n");
    }
    for (int r = 0; r < N_READS; r++) printf("read %lld %s %d %d\n", (long long) READS[r].pos, READS[r].cigar, READS[r].mapq, READS[r].flag);
    print_doubles("model_f", &fwd.match_continue, (int) (sizeof(fwd) / sizeof(double)));
    print_doubles("model_r", &rev.match_continue, (int) (sizeof(rev) / sizeof(double)));
    int tagged = 0;
    for (int c = 0; c < N_COPIES; c++) {
        printf("copy %d\nhap", c);
        for (int r = 0; r < N_READS; r++) printf(" %d", hap[c][r]);
        printf("\n");
        print_doubles("h1", h1[c], N_READS);
        print_doubles("h2", h2[c], N_READS);
        for (int r = 0; r < N_READS; r++) tagged += hap[c][r] > 0;
    }
    printf("%s: %lld chunks of %lld units each in %lld batches on %d device, %lld on the per-chunk path; %d of %d reads tagged\n", mrp_version(),
           (long long) st.chunks_per_device[0], (long long) units, (long long) st.batches, st.n_devices, (long long) st.fallback_chunks, tagged,
           N_COPIES * N_READS);
    return 0;
}
