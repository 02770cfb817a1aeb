/*
 * mrp_poa.h -- what the host half and the kernels of mrp_poa.hip share, and what the stand-alone host check
 * (tools/hostcheck/poa_host_check.cpp) reads: the per-read array, the sizing of the open-addressing tables, the record of a complete
 * indel with the key that states the reference's order of creation, and the host pass with every MRP_ERR_ARG of mrp_poa_augment
 * (DESIGN.md 9.19).  Internal.
 */
#ifndef MRP_POA_H_
#define MRP_POA_H_

#include "mrp_internal.h"

constexpr int POA_MAX_R = 255;
constexpr int64_t POA_EXACT_LIMIT = 1ll << 53; /* below it every integer is a double */
enum { POA_MATCH = 0, POA_DELETE = 1, POA_INSERT = 2 };

/* bits of the device's flag word */
constexpr uint32_t POA_FLAG_DUPLICATE = 1u << 0; /* << list: 1, 2, 4 */
constexpr uint32_t POA_FLAG_INEXACT = 1u << 3;   /* an accumulator or total of 2^53 or more */
constexpr uint32_t POA_FLAG_CAPACITY = 1u << 4;  /* the emitting pass met more than the counting pass (never: a guard on the stores) */

struct PoaRead {
    int64_t node_base;  /* node_first[c] + c: the consensus' prefix node */
    int64_t ref_base;   /* node_first[c]: its first reference symbol */
    int64_t y_off;
    int64_t table[3];   /* the first slot of the read's table of each list */
    int32_t lg[3];      /* log2 of that table's slots; -1: no table (an empty list) */
    int32_t L, y_len, shift;
    uint32_t strand;
    int32_t cons;
};

/* slots of the table of n keys, as a power of two: at least 2 n, so that a probe sequence always meets an empty slot */
inline int poa_table_lg(int64_t n) {
    if (n <= 0) return -1;
    int lg = 1;
    while ((1ll << lg) < 2 * n) lg++;
    return lg;
}

/* a match's, a delete's or an insert's key: x and y after the shift, each + 1 (a gap list's -1 becomes 0); never 0 as a whole */
__host__ __device__ inline uint64_t poa_key(int64_t x, int64_t y) { return ((uint64_t) (x + 1) << 32) | (uint64_t) (uint32_t) (y + 1); }
__host__ __device__ inline uint32_t poa_slot(uint64_t key, int lg) { return (uint32_t) ((key * 0x9E3779B97F4A7C15ull) >> (64 - lg)); }

struct PoaRecord { /* one complete insert or delete */
    uint64_t key_hi; /* read << 32 | (x + 1) for an insert, y + 1 for a delete */
    uint64_t key_lo; /* first << 32 | last: y_k, y_l of an insert, x_k, x_l of a delete */
    int32_t node;
    int32_t weight;  /* the minimum over its entries */
    uint32_t str_at; /* an insert's string in the scratch pool */
    uint32_t len;    /* an insert's symbols after the rotation; a delete's length */
    uint32_t hash;   /* of an insert's symbols and counts */
    uint32_t strand_cons; /* consensus << 1 | the read's strand */
};
__host__ __device__ inline bool poa_key_less(const PoaRecord &a, const PoaRecord &b) {
    return a.key_hi < b.key_hi || (a.key_hi == b.key_hi && a.key_lo < b.key_lo);
}

/* (mrp_poa.hip) every MRP_ERR_ARG of mrp_poa_augment that needs no device, in the order of the header; on MRP_OK reads holds one entry
 * per read with its tables sized and *table_slots their sum.  Touches no device and no output. */
int poa_check_and_build(const char *who, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first, const uint8_t *symbols,
                        const uint8_t *ref_counts, const int64_t *read_first, const uint8_t *read_symbols, const uint8_t *read_counts,
                        int64_t pool_bytes, const int64_t *y_off, const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift,
                        const mrp_posterior_pairs *matches, const mrp_posterior_pairs *deletes, const mrp_posterior_pairs *inserts,
                        const mrp_poa_options *opt, const mrp_poa *out, HostVec<PoaRead> &reads, int64_t *table_slots);

#endif
