/*
 * mrp_cross_cells.h -- the cross product of two aligned hmms in closed form (stRPHmm_createCrossProductOfTwoAlignedHmm, hmm.c:534-750;
 * why it holds: the head of mrp_engine_cross.hip): which pair of parent cells a cell of a column is, its partition, the merge cells
 * it feeds and is fed by.  Cross product and cross product + emission write the columns by it; the prune, the one-wave kernel and
 * the compaction address them by it.
 */
#ifndef MRP_CROSS_CELLS_H
#define MRP_CROSS_CELLS_H

#include "mrp_engine.h"

static __device__ __forceinline__ uint64_t accept_mask(uint32_t depth) { /* partitions.c:13-19 */
    return depth < 64 ? ~(0xFFFFFFFFFFFFFFFFull << depth) : 0xFFFFFFFFFFFFFFFFull;
}

/* Position of the pair (i, j) in the list the reference builds by visiting pairs in row-major order
 * and appending the complement pair right after each new one.  i indexes side A (Ma entries),
 * j side B (Mb entries); a side is "paired" when its entries come as (x, complement of x) at (2t, 2t+1),
 * otherwise it has exactly one, self-complementary entry. */
static __device__ __forceinline__ uint32_t pair_index(uint32_t i, uint32_t j, uint32_t Mb, bool inv, bool a_paired,
                                                      bool b_paired) {
    if (!inv) return i * Mb + j;
    if (!a_paired) return j;
    const uint32_t pj = b_paired ? (j ^ 1u) : j;
    return (i & 1u) ? (i - 1u) * Mb + 2u * pj + 1u : i * Mb + 2u * j;
}

/* The ORDER RULE of a cross product column (the one place it is written down on the device; pair_index above is its twin
 * for merge cells): cell e of the column is the pair (c1, c2) of parent cells.  Plain mode: row-major.  With inverted
 * partitions: the reference appends the complement right after every new partition, so the cells come as
 * (2r, h), (2r + 1, partner of h), (2r, h + 1), ... */
static __device__ __forceinline__ void cross_cell(uint32_t e, uint32_t C2, bool inv, bool a_cells_paired, bool b_cells_paired,
                                                  uint32_t &c1, uint32_t &c2) {
    if (!inv) { c1 = e / C2; c2 = e - c1 * C2; }
    else if (!a_cells_paired) { c1 = 0; c2 = e; }
    else {
        const uint32_t r = e / (2u * C2), t = e - r * 2u * C2, h = t >> 1;
        if (t & 1u) { c1 = 2u * r + 1u; c2 = b_cells_paired ? (h ^ 1u) : h; }
        else { c1 = 2u * r; c2 = h; }
    }
}
/* ... and the merge cells it feeds (low 16 bits) and is fed by (high 16 bits), from the parents' transitions n1, n2 */
static __device__ __forceinline__ uint32_t cross_np(const CrossCol &c, bool inv, uint32_t c1, uint32_t c2, uint32_t n1, uint32_t n2) {
    uint32_t nxt = 0, prv = 0;
    if (c.out_a != MRP_CONN_NONE) {
        const uint32_t i = c.out_a == MRP_CONN_REAL ? (n1 & 0xFFFFu) : (c.out_a == MRP_CONN_IDENT ? c1 : 0u);
        const uint32_t j = c.out_b == MRP_CONN_REAL ? (n2 & 0xFFFFu) : (c.out_b == MRP_CONN_IDENT ? c2 : 0u);
        nxt = pair_index(i, j, c.Mb, inv, (c.flags & MRP_XF_OUT_A_PAIRED) != 0, (c.flags & MRP_XF_OUT_B_PAIRED) != 0);
    }
    if (c.in_a != MRP_CONN_NONE) {
        const uint32_t i = c.in_a == MRP_CONN_REAL ? (n1 >> 16) : (c.in_a == MRP_CONN_IDENT ? c1 : 0u);
        const uint32_t j = c.in_b == MRP_CONN_REAL ? (n2 >> 16) : (c.in_b == MRP_CONN_IDENT ? c2 : 0u);
        prv = pair_index(i, j, c.Pb, inv, (c.flags & MRP_XF_IN_A_PAIRED) != 0, (c.flags & MRP_XF_IN_B_PAIRED) != 0);
    }
    return nxt | (prv << 16);
}
/* mergePartitionsOrMasks (partitions.c:21-28): side B's reads follow side A's */
static __device__ __forceinline__ uint64_t cross_partition(const CrossCol &c, uint32_t c1, uint32_t c2) {
    const uint64_t p1 = c.a_part ? c.a_part[c1] : 0ull, p2 = c.b_part ? c.b_part[c2] : 0ull;
    return c.d1 < 64 ? (p1 | (p2 << c.d1)) : p1;
}

#endif
