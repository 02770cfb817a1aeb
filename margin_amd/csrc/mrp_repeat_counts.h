/*
 * mrp_repeat_counts.h -- what the host half and the kernels of mrp_repeat_counts.hip share, and what the stand-alone host check
 * (tools/hostcheck/repeat_counts_host_check.cpp) reads: the record of an observation, the sequence number that states the definition's
 * order, the per-read array, and the host pass with every MRP_ERR_ARG of mrp_ml_repeat_counts.  Internal.
 */
#ifndef MRP_REPEAT_COUNTS_H_
#define MRP_REPEAT_COUNTS_H_

#include "mrp_internal.h"

constexpr int RC_MAX_R = 255;                   /* counts are bytes and every count >= R must stay "overlong" */
constexpr double RC_PAIR_ALIGNMENT_PROB_1 = 10000000.0;

/* bits of RcRecord::bits and of RcRead::flags */
constexpr uint32_t RC_COUNT_MASK = 0xff; /* the observed count, clamped to R - 1 (repeatSubMatrix.c:76-77) */
constexpr uint32_t RC_BELOW_R = 1u << 8; /* the raw count was below R: it takes part in min (repeatSubMatrix.c:90-99) */
constexpr uint32_t RC_STRAND = 1u << 9;  /* the read lies on the forward strand */
constexpr uint32_t RC_IN_HAP = 1u << 10; /* the read is in readsBelongingToHap1 */

struct RcRecord { /* one observation of a node, 16 B */
    double weight;
    uint32_t seq;  /* its place in the definition's order over the whole call: read-major, walk order inside the read */
    uint32_t bits;
};

struct RcRead {
    int64_t node_base; /* node_first[consensus] + x_shift: a match's x is added to it */
    int64_t y_off;
    uint32_t flags;    /* RC_STRAND | RC_IN_HAP */
    uint32_t pad;
};

/* match i of a read that owns [first, end): its sequence number.  Forward: i itself.  Backwards: the read's range mirrored, so that
 * the numbers of a call are one permutation of 0 .. matches - 1 either way. */
__host__ __device__ inline int64_t rc_sequence_number(int64_t first, int64_t end, int64_t i, int backwards) {
    return backwards ? first + (end - 1 - i) : i;
}

/* the table as the estimate kernel reads it: tt[(b * R + o) * R + u] = log_prob[(b * R + u) * R + o], so that lanes with
 * consecutive candidates u read consecutive doubles at one (b, o) */
inline void rc_transpose_table(const double *log_prob, int R, HostVec<double> &tt) {
    tt.resize((size_t) 4 * R * R);
    for (int b = 0; b < 4; b++)
        for (int u = 0; u < R; u++)
            for (int o = 0; o < R; o++) tt[((size_t) b * R + o) * R + u] = log_prob[((size_t) b * R + u) * R + o];
}

/* (mrp_repeat_counts.hip) every MRP_ERR_ARG of mrp_ml_repeat_counts, in the order of the header; on MRP_OK reads holds one entry per
 * read.  Touches no device and no output. */
int rc_check_and_build(const char *who, const double *log_prob, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first,
                       const uint8_t *symbols, const int64_t *read_first, const uint8_t *counts, int64_t counts_bytes, const int64_t *y_off,
                       const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift, const uint8_t *read_in_hap,
                       const mrp_posterior_pairs *matches, const mrp_repeat_count_options *opt, const int32_t *repeat_count_out,
                       const int64_t *non_rle_length_out, HostVec<RcRead> &reads);

#endif
