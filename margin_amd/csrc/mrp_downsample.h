/*
 * mrp_downsample.h -- what the host definition (mrp_downsample.cpp) and the kernel (mrp_downsample.hip) of the downsampling to maxDepth
 * share: the counter-based draw, the fp64 decision and a read's probability from exact integers -- one text for
 * both sides, integer work and correctly rounded fp64 operations only, so host and device agree bit for bit.
 */
#ifndef MRP_DOWNSAMPLE_H_
#define MRP_DOWNSAMPLE_H_

#include <stdint.h>

#ifdef __HIPCC__
#define MRP_DS_HD __host__ __device__
#else
#define MRP_DS_HD
#endif

/* the splitmix64 finaliser */
MRP_DS_HD inline uint64_t mrp_ds_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* u_k of a chunk: three nested finalisers, the top 53 bits times 2^-53 (the conversion and the product are exact) */
MRP_DS_HD inline double mrp_ds_draw(uint64_t seed, int64_t overlap_start, int64_t overlap_end, int64_t k) {
    const uint64_t z = mrp_ds_mix(mrp_ds_mix(mrp_ds_mix(seed ^ (uint64_t) overlap_start) ^ (uint64_t) overlap_end) ^ (uint64_t) k);
    return (double) (z >> 11) * 0x1.0p-53;
}

/* htsIntegration.c:1163-1170: averageDepth = 1.0 * totalVcfEntries / chunkSize; "averageDepth < intendedDepth" returns FALSE.  V == 0
 * gives inf or nan, which is never below D: the chunk falls through to :1174 */
MRP_DS_HD inline bool mrp_ds_shallow(int64_t total, int64_t V, int64_t D) { return 1.0 * (double) total / (double) V < (double) D; }

/* p of a read with l > 0 in a downsampled chunk with total > T: B = the l of the reads ordered before it */
MRP_DS_HD inline double mrp_ds_prob(int64_t B, int64_t l, int64_t T) {
    if (B + l <= T) return 1.0;
    if (B < T) return (double) (T - B) / (double) l; /* both below 2^31: exact in fp64, the quotient correctly rounded */
    return 0.0;
}

/* read j is ordered before read i (both with l > 0): h_j / l_j > h_i / l_i, equal ratios by ascending read index */
MRP_DS_HD inline bool mrp_ds_before(int32_t hj, int32_t lj, int64_t j, int32_t hi, int32_t li, int64_t i) {
    const int64_t a = (int64_t) hj * li, b = (int64_t) hi * lj;
    return a > b || (a == b && j < i);
}

#endif
