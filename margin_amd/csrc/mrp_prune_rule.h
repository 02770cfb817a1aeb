/*
 * mrp_prune_rule.h -- what the prune kernel (mrp_engine_kernels.hip) and the one-wave kernel (mrp_engine_small.hip) share of
 * stRPHmm_pruneForwards (hmm.c:1049-1109): how many candidates a column keeps, and the integer a posterior is ranked by.
 */
#ifndef MRP_PRUNE_RULE_H
#define MRP_PRUNE_RULE_H

#include "mrp_engine.h" /* MRP_ENGINE_ERR_POSTERIOR; MRP_NEG_I32 through mrp_kernels.h */

/* n kept of n_link candidates whose first g pass the posterior threshold: the loop of hmm.c:1073-1079 /
 * :1094-1100 ("while n > min && (n > max || last.posterior < threshold) drop last") in closed form */
static __device__ __forceinline__ int kept_count(int n_link, int g, int min_p, int max_p) {
    if (n_link <= min_p) return n_link;
    int n = g < max_p ? g : max_p;
    return n > min_p ? n : min_p;
}

/* posterior bin of a cell or merge cell: total - f - b, all three exact integers below 2^30 in magnitude (the int32
 * recursion kernel only takes hmms whose cost bound is below 2^30, and f + b counts every column at most once), so the
 * difference is formed in 32 bits -- in 64 bits the compiler widens every f and b it holds in registers */
static __device__ __forceinline__ int posterior_bin(int32_t f, int32_t b, int32_t total, int n_bins, int *errbits) {
    if (f == MRP_NEG_I32 || b == MRP_NEG_I32) return n_bins - 1; /* exp(-inf) = 0 */
    const int32_t s = total - f - b;
    if (s < 0) { *errbits |= MRP_ENGINE_ERR_POSTERIOR; return 0; }
    return s < n_bins - 1 ? (int) s : n_bins - 1;
}

#endif
