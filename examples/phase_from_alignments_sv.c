/*
 * phase_from_alignments_sv.c -- the first step of margin phase's chunk loop under params/phase/allParams.phase_vcf.ont.sv.json
 * (indelSizeForSVHandling = 50) from plain C:
 *
 *   alignments + VCF entries --mrp_mark_structural_variants, mrp_extract_read_substrings--> read substrings at the variants
 *
 * With indelSizeForSVHandling > 0 the reference walks the small variants and the structural ones separately and merges the two
 * results per read (htsIntegration.c:1722-1759).  The library refuses that mode until the context admits it
 * (mrp_context_set_sv_split); mrp_haplotag_aligned_chunks and mrp_phase_aligned_chunks(_with_filtered) honour the same switch.
 * The input is one small hand-made chunk: a 40-base reference slice at genome 100, a SNP at 118 (window [16, 21]) listed before a
 * 60-base insertion at 120 (window [14, 27]), a dozen reads whose bases cycle A C G T.  In the one-list walk the insertion's
 * substring would start where the SNP's does, at 16; in its own walk it starts at 14.  Prints the input (so that a caller in
 * another language can rebuild it) and per variant its entries as read:length.
 *
 *   gcc -O2 -Iinclude examples/phase_from_alignments_sv.c -Lmargin_amd/lib -lmargin_rphmm -lm -Wl,-rpath,$PWD/margin_amd/lib -o phase_from_alignments_sv
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

enum { N_VARIANTS = 2, N_ALLELES = 4, N_READS = 12, MAX_OPS = 8, INDEL_SIZE_FOR_SV_HANDLING = 50 };

static const char REFERENCE[] = "ACGTTGCAACACGTTGCAACACGTTGCAACACGTTGCAAC"; /* genome 100..139 */
static const int64_t VARIANT_POS[N_VARIANTS] = {118, 120};
static const int64_t ALLELE_FIRST[N_VARIANTS + 1] = {0, 2, 4};
static const char *ALLELES[N_ALLELES] = {"A", "G", /* allele 0 of a variant = REF */
                                         "A", "AGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATTACAGATT"};
static const struct { int64_t pos; const char *cigar; uint8_t mapq; uint16_t flag; } READS[N_READS] = {
    {100, "30M", 60, 0},      {100, "40M", 60, 0x10},  {101, "29M", 60, 0},     {105, "3S25M", 60, 0x10}, {102, "12M2I14M", 60, 0}, {104, "8M3D15M", 60, 0x10},
    {100, "40M", 3, 0},       {115, "20M", 60, 0},     {119, "20M", 60, 0x10},  {121, "15M", 60, 0},      {100, "16M1I12M", 60, 0}, {100, "30M", 60, 0x100},
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

int main(void) {
    mrp_context *ctx = NULL;
    CHECK(mrp_context_create(0, &ctx));
    CHECK(mrp_context_set_sv_split(ctx, 1)); /* off by default: indel_size_for_sv_handling != 0 is then MRP_ERR_UNSUPPORTED */

    /* the chunk as htslib holds it: alleles as chars in one buffer, CIGARs as BAM words, bases as 4-bit codes (A C G T = 1 2 4 8) */
    char allele_chars[128];
    int64_t allele_off[N_ALLELES];
    int32_t allele_len[N_ALLELES];
    int64_t at = 0;
    for (int a = 0; a < N_ALLELES; a++) {
        allele_off[a] = at;
        allele_len[a] = (int32_t) strlen(ALLELES[a]);
        memcpy(allele_chars + at, ALLELES[a], (size_t) allele_len[a]);
        at += allele_len[a];
    }
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
    chunk.n_reads = N_READS;
    chunk.pos = pos;
    chunk.flag = flag;
    chunk.mapq = mapq;
    chunk.l_qseq = l_qseq;
    chunk.cigar_first = cigar_first;
    chunk.cigar = cigar;
    chunk.seq_first = seq_first;
    chunk.seq = seq;
    /* isStructuralVariant as the VCF loader sets it (vcf.c:173-185): an allele longer than indelSizeForSVHandling */
    uint8_t is_sv[N_VARIANTS];
    CHECK(mrp_mark_structural_variants(&chunk, INDEL_SIZE_FOR_SV_HANDLING, is_sv));
    chunk.is_sv = is_sv;

    /* small windows, as the reference slice is small; indelSizeForSVHandling as in the SV configuration; everything else as shipped */
    const mrp_extract_options options = {2, 6, 5, 0, 0, INDEL_SIZE_FOR_SV_HANDLING, 0};
    mrp_extracted_chunk *x = NULL;
    CHECK(mrp_extract_read_substrings(ctx, 1, &chunk, &options, &x, NULL));

    for (int v = 0; v < N_VARIANTS; v++) {
        printf("variant %lld %d", (long long) VARIANT_POS[v], is_sv[v]);
        for (int64_t a = ALLELE_FIRST[v]; a < ALLELE_FIRST[v + 1]; a++) printf(" %s", ALLELES[a]);
        printf("\n");
    }
    for (int r = 0; r < N_READS; r++) printf("read %lld %s %d %d\n", (long long) READS[r].pos, READS[r].cigar, READS[r].mapq, READS[r].flag);
    printf("status");
    for (int r = 0; r < N_READS; r++) printf(" %d", x->read_status[r]);
    printf("\n");
    for (int v = 0; v < N_VARIANTS; v++) {
        printf("entries %d window %lld %lld:", v, (long long) x->ref_aln_start[v], (long long) x->ref_aln_stop_incl[v]);
        for (int64_t e = x->entry_first[v]; e < x->entry_first[v + 1]; e++) printf(" %d:%d", x->entry_read[e], x->entry_len[e]);
        printf("\n");
    }
    printf("%lld substrings at %d variants, %d structural\n", (long long) x->entry_first[N_VARIANTS], N_VARIANTS, is_sv[0] + is_sv[1]);

    void *arrays[] = {x->ref_aln_start, x->ref_aln_stop_incl, x->allele_first, x->allele_off, x->allele_len, x->read_status, x->read_n_substrings,
                      x->entry_first, x->entry_read, x->entry_off, x->entry_len, x->pool};
    for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); i++) mrp_free(arrays[i]);
    mrp_free(x);
    mrp_context_destroy(ctx);
    return 0;
}
