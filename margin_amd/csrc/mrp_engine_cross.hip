/*
 * mrp_engine_cross.hip -- the cross product of a device-resident merge level, and the cross product + emission in
 * one pass.  A level's other stages: mrp_engine_layout.hip, mrp_engine_kernels.hip (prune), mrp_engine_small.hip, mrp_engine_final.hip.
 *
 *  mrp_cross_kernel    stRPHmm_createCrossProductOfTwoAlignedHmm (hmm.c:534-750) in closed form.
 *                      The reference builds each column by hashing merged partitions in (c1, c2)
 *                      row-major order and, with includeInvertedPartitions, appending the complement
 *                      right after every new partition (hmm.c:627-655; merge cells :686-740).  When the
 *                      two parents keep their cells / merge cells in adjacent complement pairs (they do
 *                      by construction: hmm.c:97-133 builds {1, 0}, the prune keeps both or neither of a
 *                      pair and its sort is stable) the resulting order is a pure function of the index
 *                      pair, so a cell's partition and the indices of the merge cells it feeds / is fed
 *                      by are computed without any hash table (mrp_cross_cells.h).  The kernel VERIFIES the
 *                      pair order of every parent column it reads and raises MRP_ENGINE_ERR_STRUCTURE otherwise
 *                      (the host then redoes the chunk through the hashing path of rphmm_host.c).
 */
#include <type_traits>

#include "mrp_engine.h"
#include "mrp_level_order.h" /* cross_emit_plan */
#include "mrp_cross_cells.h"
#include "mrp_wave.h"

static __device__ int verify_side(const uint64_t *part, const uint32_t *np, uint32_t C, uint32_t depth, uint32_t M_out,
                                  uint32_t M_in, uint32_t out_kind, uint32_t in_kind, bool inv, bool out_paired,
                                  bool in_paired, uint32_t tid, uint32_t nt) {
    if (!part) return 0;
    int bad = 0;
    const bool cells_paired = inv && depth > 0;
    if (cells_paired && (C & 1u)) return MRP_ENGINE_ERR_STRUCTURE;
    const uint64_t acc = accept_mask(depth);
    for (uint32_t e = tid; e < C; e += nt) {
        const uint32_t v = np[e], nx = v & 0xFFFFu, pv = v >> 16;
        uint32_t vo = v;
        if (cells_paired) {
            if (part[e ^ 1u] != (~part[e] & acc)) bad |= MRP_ENGINE_ERR_STRUCTURE;
            vo = np[e ^ 1u];
        }
        if (out_kind == MRP_CONN_REAL) {
            if (nx >= M_out) bad |= MRP_ENGINE_ERR_RANGE;
            if (inv) {
                if (out_paired) { if ((M_out & 1u) || (vo & 0xFFFFu) != (nx ^ 1u)) bad |= MRP_ENGINE_ERR_STRUCTURE; }
                else if (M_out != 1u) bad |= MRP_ENGINE_ERR_STRUCTURE;
            }
        }
        if (in_kind == MRP_CONN_REAL) {
            if (pv >= M_in) bad |= MRP_ENGINE_ERR_RANGE;
            if (inv) {
                if (in_paired) { if ((M_in & 1u) || (vo >> 16) != (pv ^ 1u)) bad |= MRP_ENGINE_ERR_STRUCTURE; }
                else if (M_in != 1u) bad |= MRP_ENGINE_ERR_STRUCTURE;
            }
        }
    }
    return bad;
}

__global__ void __launch_bounds__(256) mrp_cross_kernel(const CrossCol *__restrict__ cols, int64_t n_cols,
                                                        uint64_t *__restrict__ partition, uint32_t *__restrict__ cell_np,
                                                        int32_t *__restrict__ err, const int32_t *__restrict__ col_hmm,
                                                        int32_t *__restrict__ err_hmm) {
    for (int64_t col = blockIdx.x; col < n_cols; col += gridDim.x) {
        const CrossCol c = k_load(cols + col);
        const bool inv = (c.flags & MRP_XF_INVERTED) != 0;
        const uint32_t C1 = c.C1, C2 = c.C2, C = C1 * C2;
        const bool a_cells_paired = inv && c.a_part && c.d1 > 0, b_cells_paired = inv && c.b_part && c.d2 > 0;
        int bad = verify_side(c.a_part, c.a_np, C1, c.d1, c.Ma, c.Pa, c.out_a, c.in_a, inv,
                              (c.flags & MRP_XF_OUT_A_PAIRED) != 0, (c.flags & MRP_XF_IN_A_PAIRED) != 0, threadIdx.x, blockDim.x);
        bad |= verify_side(c.b_part, c.b_np, C2, c.d2, c.Mb, c.Pb, c.out_b, c.in_b, inv,
                           (c.flags & MRP_XF_OUT_B_PAIRED) != 0, (c.flags & MRP_XF_IN_B_PAIRED) != 0, threadIdx.x, blockDim.x);
        if ((!c.a_part && C1 != 1u) || (!c.b_part && C2 != 1u)) bad |= MRP_ENGINE_ERR_RANGE;
        if (bad) { atomicOr(err, bad); atomicOr(err_hmm + col_hmm[col], bad); }
        if (__syncthreads_or(bad)) { /* the level is discarded by the host; keep the arrays defined meanwhile */
            for (uint32_t e = threadIdx.x; e < C; e += blockDim.x) {
                partition[c.x_cell_off + e] = 0ull;
                cell_np[c.x_cell_off + e] = 0u;
            }
            continue;
        }
        for (uint32_t e = threadIdx.x; e < C; e += blockDim.x) {
            uint32_t c1, c2;
            cross_cell(e, C2, inv, a_cells_paired, b_cells_paired, c1, c2);
            const uint32_t n1 = c.a_part ? c.a_np[c1] : 0u, n2 = c.b_part ? c.b_np[c2] : 0u;
            partition[c.x_cell_off + e] = cross_partition(c, c1, c2);
            cell_np[c.x_cell_off + e] = cross_np(c, inv, c1, c2, n1, n2);
        }
    }
}

hipError_t mrp_launch_cross(const CrossCol *cols_dev, int64_t n_cols, uint64_t *partition, uint32_t *cell_np, int32_t *err,
                            const int32_t *col_hmm_dev, int32_t *err_hmm, hipStream_t stream, LaunchCensus *census) {
    if (n_cols <= 0) return hipSuccess;
    if (census) census->bump(CENSUS_CROSS_TWO_KERNELS);
    const int64_t grid = n_cols < 65536 ? n_cols : 65536;
    hipLaunchKernelGGL(mrp_cross_kernel, dim3((unsigned) grid), dim3(256), 0, stream, cols_dev, n_cols, partition, cell_np, err, col_hmm_dev,
                       err_hmm);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------------------------ */
/* cross product + emission in one pass (merge levels, no ancestor substitution model)          */
/* ------------------------------------------------------------------------------------------ */
/*
 * emissionLogProbability (emissions.c:221-240) of a cross product cell WITHOUT its partition ever being written: the cell
 * (c1, c2) holds the reads of parent cell c1 followed by those of parent cell c2 (partitions.c:21-28), and
 * getLogProbOfAllele (emissions.c:125-138) is a sum over the reads of the partition, so per allele slot
 *      hap1(c1, c2) = tA[slot][c1] + tB[slot][c2],   hap2 = T[slot] - hap1          (emissions.c:144-154)
 * with tA / tB the per-parent-cell sums over the side's own reads: (C1 + C2) * slots dot products per column instead of
 * C1 * C2 * slots.  One wave per column.  The tables sit in LDS as packed 16-bit halves, one 16-byte aligned row per parent cell,
 *      A[c1][slot] = tA | (T - tA) << 16        B[c2][slot] = tB - (tB << 16)
 * so that ONE 32-bit add yields hap1 in the low and hap2 in the high half (no carry crosses: both are sums of at most 64
 * bytes), and one v_pk_min_u16 keeps both running minima over the alleles of a site (emissions.c:174-185, :205-207).
 * With inverted partitions cells 2q, 2q+1 are complements and share their cost (hap1 <-> hap2): a lane computes it once.
 * HBM traffic: 8 B written per cell (cost + transitions), nothing read per cell.
 */
#define XE_WAVES 1
/* Table dwords per wave, chosen per launch (dynamic LDS): XE_CAP_NARROW for the levels whose columns all take the table-free path
 * below (200 parent cells x 4 allele slots would still fit: a column that needs the tables after all fills them several times) --
 * 6.4 KB per one-wave workgroup, the registers' 20 waves per CU fit; XE_CAP_WIDE where two pruned columns of 100 cells meet: 8 slots
 * = 4 biallelic sites per fill instead of 2 (a column of more sites walks its cells once per fill, adding to the costs already
 * stored), 9.7 KB, 16 waves per CU.  Measured per 96-chunk batch, widest level / the two above it / the three below it:
 * 832 dwords 1.39 / 0.65 + 0.48 / 0.37-0.39 ms; 1 248: 1.24 / 0.64 + 0.49 / 0.39-0.41; 1 664: 1.06 / 0.60 + 0.48 / 0.35-0.44;
 * 2 496: 1.16 / 0.78 + 0.47 / 0.48-0.59; 3 328: 1.26 / 0.84 + 0.58 / 0.54-0.69. */
#define XE_CAP_NARROW 832
#define XE_CAP_WIDE 1664
#define XE_ROWS 16 /* allele slots staged per table fill */

typedef unsigned short xe_u16x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    const xe_u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(xe_u16x2, a), __builtin_bit_cast(xe_u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
/* sum of the profile bytes of the reads in P over one allele slot: bytes are packed four reads to a word */
template <typename RowPtr>
static __device__ __forceinline__ uint32_t slot_dot(RowPtr row, uint64_t P, int w4_lo, int w4_hi) {
    uint32_t sum = 0;
    for (int w4 = w4_lo; w4 < w4_hi; w4++) {
        const uint4 bts = *reinterpret_cast<const uint4 *>(row + 4 * w4);
        const uint32_t bits = (uint32_t) (P >> (16 * w4)) & 0xFFFFu;
        sum = __builtin_amdgcn_udot4(bts.x, ((bits & 0xFu) * 0x00204081u) & 0x01010101u, sum, false);
        sum = __builtin_amdgcn_udot4(bts.y, (((bits >> 4) & 0xFu) * 0x00204081u) & 0x01010101u, sum, false);
        sum = __builtin_amdgcn_udot4(bts.z, (((bits >> 8) & 0xFu) * 0x00204081u) & 0x01010101u, sum, false);
        sum = __builtin_amdgcn_udot4(bts.w, ((bits >> 12) * 0x00204081u) & 0x01010101u, sum, false);
    }
    return sum;
}

/* cost of one cell over the sites of the tables: per site min over alleles of hap1 plus min over alleles of hap2.
 * pa, pb: the cell's two table rows (slot-minor, 16-byte aligned): four slots per LDS read. */
static __device__ __forceinline__ uint32_t xe_cost(const uint32_t *pa, const uint32_t *pb, uint32_t nsl, uint64_t ends) {
    uint32_t cost = 0, m = 0xFFFFFFFFu;
    for (uint32_t s4 = 0; s4 < nsl; s4 += 4u) {
        const uint4 a = *reinterpret_cast<const uint4 *>(pa + s4), b = *reinterpret_cast<const uint4 *>(pb + s4);
        const uint32_t x[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
        const uint32_t e4 = (uint32_t) (ends >> s4) & 0xFu, left = nsl - s4; /* wave-uniform */
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if ((uint32_t) j < left) {
                m = pk_min_u16(m, x[j]);
                if (e4 & (1u << j)) { cost += (m & 0xFFFFu) + (m >> 16); m = 0xFFFFFFFFu; }
            }
        }
    }
    return cost;
}
/* Table rows of one side for columns with many parent cells: a lane owns a parent cell (its partition's read bits are
 * expanded to 0/1 bytes once); the packed bytes of a slot were staged in LDS and every lane reads the same words.
 * NW4 = 16-read groups the side's reads span; the partition is shifted up to the merged column's read positions, then down
 * by the first group (rowbuf points at that group's words). */
template <int NW4, bool SIDE_B>
static __device__ __forceinline__ void xe_fill_side(uint32_t *rows, uint32_t ST, uint64_t P0, uint64_t P1, uint32_t C, uint32_t up,
                                                    uint32_t down, uint32_t nsl, const uint32_t *rowbuf, const uint32_t *totbuf, int lane) {
    /* the partitions of parent cells lane and lane + 64 are in the lane's registers (P0, P1: requested with everything else
     * the column needs, right after its descriptor) */
    for (uint32_t u = 0; u * WAVE < C; u++) {
        const uint32_t cc = (uint32_t) lane + u * WAVE;
        const bool act = cc < C;
        uint64_t P = act ? (u ? P1 : P0) : 0ull;
        P = up < 64u ? (P << up) >> down : 0ull;
        uint32_t sel[4 * NW4];
#pragma unroll
        for (int w = 0; w < 4 * NW4; w++) sel[w] = ((uint32_t) ((P >> (4 * w)) & 0xFull) * 0x00204081u) & 0x01010101u;
        for (uint32_t slot = 0; slot < nsl; slot++) {
            uint32_t t = 0;
#pragma unroll
            for (int k = 0; k < NW4; k++) {
                const uint4 r = *reinterpret_cast<const uint4 *>(rowbuf + slot * 16 + 4 * k);
                t = __builtin_amdgcn_udot4(r.x, sel[4 * k], t, false);
                t = __builtin_amdgcn_udot4(r.y, sel[4 * k + 1], t, false);
                t = __builtin_amdgcn_udot4(r.z, sel[4 * k + 2], t, false);
                t = __builtin_amdgcn_udot4(r.w, sel[4 * k + 3], t, false);
            }
            if (act) rows[cc * ST + slot] = SIDE_B ? t - (t << 16) : (t | ((totbuf[slot] - t) << 16));
        }
    }
}

/* pair_index (the merge cell a cell feeds / is fed by) split into a term per parent cell of side A and two per parent cell of
 * side B, computed once per parent cell instead of once per cell:
 *      index(c1, c2) = base(c1) + (sel(c1) ? B1(c2) : B0(c2))
 * tra[c1] = {out: base | sel << 31, in: base | sel << 31},  trb[c2] = {out: B0 | B1 << 16, in: B0 | B1 << 16}. */
static __device__ __forceinline__ uint32_t xe_term_a(uint32_t kind, bool none, uint32_t n_idx, uint32_t c1, uint32_t Mb, bool inv, bool a_paired) {
    const uint32_t i = kind == MRP_CONN_REAL ? n_idx : (kind == MRP_CONN_IDENT ? c1 : 0u);
    if (none) return 0u;
    if (!inv) return i * Mb;
    if (!a_paired) return 0u;
    return (i & 1u) ? (((i - 1u) * Mb + 1u) | 0x80000000u) : i * Mb;
}
static __device__ __forceinline__ uint32_t xe_term_b(uint32_t kind, bool none, uint32_t n_idx, uint32_t c2, bool inv, bool a_paired, bool b_paired) {
    const uint32_t j = kind == MRP_CONN_REAL ? n_idx : (kind == MRP_CONN_IDENT ? c2 : 0u);
    if (none) return 0u;
    if (!inv || !a_paired) return j | (j << 16);
    return (2u * j) | ((2u * (b_paired ? (j ^ 1u) : j)) << 16);
}
/* np0, np1: the transitions of parent cells lane and lane + 64 of each side (registers) */
static __device__ __forceinline__ void xe_stage_transitions(const CrossCol &c, bool inv, uint2 *tra, uint2 *trb, int lane, const uint32_t *npa,
                                                            const uint32_t *npb) {
    const bool oap = (c.flags & MRP_XF_OUT_A_PAIRED) != 0, obp = (c.flags & MRP_XF_OUT_B_PAIRED) != 0;
    const bool iap = (c.flags & MRP_XF_IN_A_PAIRED) != 0, ibp = (c.flags & MRP_XF_IN_B_PAIRED) != 0;
    const bool no_out = c.out_a == MRP_CONN_NONE, no_in = c.in_a == MRP_CONN_NONE;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const uint32_t i = (uint32_t) lane + (uint32_t) u * WAVE;
        if (i < min((uint32_t) c.C1, 128u))
            tra[i] = make_uint2(xe_term_a(c.out_a, no_out, npa[u] & 0xFFFFu, i, c.Mb, inv, oap), xe_term_a(c.in_a, no_in, npa[u] >> 16, i, c.Pb, inv, iap));
        if (i < min((uint32_t) c.C2, 128u))
            trb[i] = make_uint2(xe_term_b(c.out_b, no_out, npb[u] & 0xFFFFu, i, inv, oap, obp), xe_term_b(c.in_b, no_in, npb[u] >> 16, i, inv, iap, ibp));
    }
}
/* verify_side over a side of at most 128 parent cells held in registers (entry e = lane + 64 u; its complement e ^ 1 sits in
 * the neighbouring lane) */
template <int NU = 2>
static __device__ __forceinline__ int xe_verify_side(bool have, const uint64_t *P, const uint32_t *np, uint32_t C, uint32_t depth, uint32_t M_out,
                                                     uint32_t M_in, uint32_t out_kind, uint32_t in_kind, bool inv, bool out_paired, bool in_paired,
                                                     int lane) {
    if (!have) return 0;
    int bad = 0;
    const bool cells_paired = inv && depth > 0;
    if (cells_paired && (C & 1u)) return MRP_ENGINE_ERR_STRUCTURE;
    const uint64_t acc = accept_mask(depth);
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const uint32_t e = (uint32_t) lane + (uint32_t) u * WAVE;
        const uint32_t v = np[u], nx = v & 0xFFFFu, pv = v >> 16;
        const uint32_t v_other = (uint32_t) __shfl_xor((int) v, 1, WAVE);
        const uint64_t p_other = ((uint64_t) (uint32_t) __shfl_xor((int) (uint32_t) (P[u] >> 32), 1, WAVE) << 32) |
                                 (uint32_t) __shfl_xor((int) (uint32_t) P[u], 1, WAVE);
        if (e >= C) continue;
        uint32_t vo = v;
        if (cells_paired) {
            if (p_other != (~P[u] & acc)) bad |= MRP_ENGINE_ERR_STRUCTURE;
            vo = v_other;
        }
        if (out_kind == MRP_CONN_REAL) {
            if (nx >= M_out) bad |= MRP_ENGINE_ERR_RANGE;
            if (inv) {
                if (out_paired) { if ((M_out & 1u) || (vo & 0xFFFFu) != (nx ^ 1u)) bad |= MRP_ENGINE_ERR_STRUCTURE; }
                else if (M_out != 1u) bad |= MRP_ENGINE_ERR_STRUCTURE;
            }
        }
        if (in_kind == MRP_CONN_REAL) {
            if (pv >= M_in) bad |= MRP_ENGINE_ERR_RANGE;
            if (inv) {
                if (in_paired) { if ((M_in & 1u) || (vo >> 16) != (pv ^ 1u)) bad |= MRP_ENGINE_ERR_STRUCTURE; }
                else if (M_in != 1u) bad |= MRP_ENGINE_ERR_STRUCTURE;
            }
        }
    }
    return bad;
}
static __device__ __forceinline__ uint32_t xe_np(uint2 a, uint2 b) { /* next | prev << 16 */
    const uint32_t nxt = (a.x & 0x7FFFFFFFu) + ((int32_t) a.x < 0 ? b.x >> 16 : b.x & 0xFFFFu);
    const uint32_t prv = (a.y & 0x7FFFFFFFu) + ((int32_t) a.y < 0 ? b.y >> 16 : b.y & 0xFFFFu);
    return nxt | (prv << 16);
}

/* ---- narrow columns: at most 64 array entries and at most 64 parent cells per side (the first merge levels: a few cells per
 * column, long runs of sites) ----
 * No tables: entry `lane` of the column is a cell (c1, c2) whose merged partition P the lane holds; its cost over one allele slot is
 * getLogProbOfAllele (emissions.c:125-138) evaluated directly, Sum_w v_dot4(bytes of reads 4w..4w+3, bits of P expanded to 0/1
 * bytes).  The packed bytes of a slot are the same 64 bytes for every lane.  A chunk of up to 16 slots (whole sites) is requested
 * at once: FOUR coalesced loads -- lane l of load g holds dword l & 15 of slot 4 g + (l >> 4) -- and one for the byte sums, all in
 * flight together (one round trip per 16 slots; scalar loads, tried first, return out of order and the compiler waits for each
 * slot's row in turn); a slot's words then reach every lane through v_readlane (wave-uniform operands of the v_dot4).  Per site the
 * minima over its alleles of hap1 and of hap2 = total - hap1 (emissions.c:144-154, :174-185, :205-207).  With the table kernel a
 * column of the first merge levels cost ~1 900 instructions whatever its cells (two table fills through LDS, transition terms, a
 * grid walk), two thirds of them on the scalar unit; this path has neither LDS traffic nor a second pass. */
/* The same cost with the lanes along the SLOTS (biallelic sites, a column of few cells and many sites: the first merge level's
 * columns hold two to four cells and up to sixty sites): lane l keeps the packed bytes of slot l of a chunk of 64 -- every lane its own
 * 16 x NW4 bytes, the wave a contiguous 4 KB --; for each cell of the column (its partition broadcast through a scalar pair) one
 * v_dot4 chain per lane gives hap1 of all 64 slots at once, the two alleles of a site sit in neighbouring lanes (one DPP swap for the
 * minima) and the sites are summed across the wave.  Per cell and 32 sites some 35 instructions, where a lane per cell takes 17 per
 * slot.  Returns, in lane e, the cost of cell e over the chunk. */
static __device__ __forceinline__ uint32_t xe_wave_sum_u32(uint32_t v) {
    return (uint32_t) __builtin_amdgcn_readlane(wave_incl_scan_bc((int) v), WAVE - 1); /* the last lane of the DPP scan holds the sum */
}
template <int NW4>
static __device__ __forceinline__ uint32_t xe_slots_chunk(const uint32_t *__restrict__ slot_bytes, const uint32_t *__restrict__ slot_total, int64_t slot0,
                                                          uint32_t nsl, uint32_t U, uint64_t P, int lane) {
    const bool have = (uint32_t) lane < nsl;
    const uint4 *rp = reinterpret_cast<const uint4 *>(slot_bytes + (slot0 + (have ? (uint32_t) lane : 0u)) * 16);
    uint4 row[NW4];
#pragma unroll
    for (int k = 0; k < NW4; k++) row[k] = rp[k];
    const uint32_t tot = slot_total[slot0 + (have ? (uint32_t) lane : 0u)];
    uint32_t mine = 0;
    for (uint32_t e = 0; e < U; e++) { /* wave-uniform */
        const uint64_t Pe = ((uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (P >> 32), (int) e) << 32) |
                            (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) P, (int) e);
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < NW4; k++) {
            const uint32_t bits = (uint32_t) (Pe >> (16 * k)) & 0xFFFFu; /* scalar: the expansion runs on the scalar unit */
            t = __builtin_amdgcn_udot4(row[k].x, ((bits & 0xFu) * 0x00204081u) & 0x01010101u, t, false);
            t = __builtin_amdgcn_udot4(row[k].y, (((bits >> 4) & 0xFu) * 0x00204081u) & 0x01010101u, t, false);
            t = __builtin_amdgcn_udot4(row[k].z, (((bits >> 8) & 0xFu) * 0x00204081u) & 0x01010101u, t, false);
            t = __builtin_amdgcn_udot4(row[k].w, ((bits >> 12) * 0x00204081u) & 0x01010101u, t, false);
        }
        const uint32_t h2 = tot - t;
        const uint32_t o1 = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) t, 0xB1, 0xf, 0xf, false);  /* quad_perm [1,0,3,2]: the site's other allele */
        const uint32_t o2 = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) h2, 0xB1, 0xf, 0xf, false);
        const uint32_t v = (have && (lane & 1) == 0) ? min(t, o1) + min(h2, o2) : 0u;
        const uint32_t sum = xe_wave_sum_u32(v);
        mine += (uint32_t) lane == e ? sum : 0u;
    }
    return mine;
}

template <int NW4>
static __device__ __forceinline__ uint32_t xe_narrow_chunk(const uint32_t *__restrict__ slot_bytes, const uint32_t *__restrict__ slot_total, int64_t slot0,
                                                           uint32_t nsl, uint32_t ends, const uint32_t (&sel)[16], int lane, uint32_t &m1, uint32_t &m2) {
    const uint32_t grp = (uint32_t) lane >> 4, dw = (uint32_t) lane & 15u;
    uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 4; g++)
        if (4u * (uint32_t) g < nsl) r[g] = slot_bytes[(slot0 + min(4u * (uint32_t) g + grp, nsl - 1u)) * 16 + dw];
    const uint32_t tot_v = slot_total[slot0 + min((uint32_t) lane, nsl - 1u)];
    uint32_t cost = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        if (4u * (uint32_t) g < nsl) { /* wave-uniform */
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t sidx = 4u * (uint32_t) g + (uint32_t) j;
                const bool valid = sidx < nsl;
                const bool last = valid && ((ends >> sidx) & 1u) != 0u;
                uint32_t t = 0;
#pragma unroll
                for (int k = 0; k < 4 * NW4; k++) t = __builtin_amdgcn_udot4((uint32_t) __builtin_amdgcn_readlane((int) r[g], j * 16 + k), sel[k], t, false);
                const uint32_t tt = (uint32_t) __builtin_amdgcn_readlane((int) tot_v, g * 4 + j);
                const uint32_t n1 = min(m1, t), n2 = min(m2, tt - t);
                m1 = valid ? n1 : m1;
                m2 = valid ? n2 : m2;
                cost += last ? m1 + m2 : 0u;
                m1 = last ? 0xFFFFFFFFu : m1;
                m2 = last ? 0xFFFFFFFFu : m2;
            }
        }
    }
    return cost;
}

#ifdef XE_CLOCK /* development: where a wave of mrp_cross_emit_kernel spends its time (summed over the waves of a launch, clock ticks) */
#define XE_T(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); xe_sec[i] += t_ - xe_t; xe_t = t_; } while (0)
#else
#define XE_T(i) do { } while (0)
#endif
struct __attribute__((packed, aligned(4))) xe_u32x4 { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(4))) xe_u32x2 { uint32_t x, y; };

#define XE_MIN_WAVES 1
/* MODE 1: the narrow columns only (no tables, no LDS, two thirds of the registers: eight waves per SIMD wait for their descriptors and
 * parent cells side by side); MODE 2: the columns that need the tables; a wave that meets a column of the other kind ends behind the
 * column's descriptor.  MODE 0: both kinds in one launch.  The first merge levels, whose hmms are nearly all small, take MODE 1 (and
 * MODE 2 behind it unless the static bounds say every column is narrow); the levels of wide columns take MODE 0 -- a pass of waves
 * that only skip costs them 70-90 us per 190 000 columns, more than their few narrow columns gain from the leaner kernel. */
template <int MODE>
__global__ void __launch_bounds__(XE_WAVES * WAVE, MODE == 1 ? 8 : XE_MIN_WAVES) mrp_cross_emit_kernel(const CrossCol *__restrict__ ccols, const DevCol *__restrict__ cols,
                                                                         const DevChunk *__restrict__ chunks, int64_t n_cols,
                                                                         const uint32_t *__restrict__ slot_bytes,
                                                                         const uint32_t *__restrict__ slot_total,
                                                                         uint32_t *__restrict__ cell_np, uint32_t *__restrict__ cell_cost,
                                                                         int32_t *__restrict__ err, const int32_t *__restrict__ col_hmm,
                                                                         int32_t *__restrict__ err_hmm, uint32_t cap) {
    /* per wave: tables [cap] | packed bytes of a fill [XE_ROWS * 16] | their byte sums [XE_ROWS] | transition terms of the parent cells
     * [256 uint2], see xe_stage_transitions */
    extern __shared__ __attribute__((aligned(16))) uint32_t xe_lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x / WAVE));
    uint32_t *tab = xe_lds + (size_t) wave * (cap + XE_ROWS * 16 + XE_ROWS + 512), *rowbuf = tab + cap, *totbuf = rowbuf + XE_ROWS * 16;
    uint2 *tra = reinterpret_cast<uint2 *>(totbuf + XE_ROWS), *trb = tra + 128;
#ifdef XE_CLOCK
    uint64_t xe_sec[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xe_t = __builtin_amdgcn_s_memtime();
#endif
    for (int64_t col = (int64_t) blockIdx.x * XE_WAVES + wave; col < n_cols; col += (int64_t) gridDim.x * XE_WAVES) {
        const CrossCol c = k_load(ccols + col);
        const DevCol dc = k_load(cols + col);
#ifdef XE_CLOCK
        if (c.x_cell_off == -0x123456789LL || dc.slot_off == -0x123456789LL) continue; /* (uses the descriptors: the wait for them is section 0) */
        XE_T(0);
        xe_sec[7] += 1;
#endif
        const bool inv = (c.flags & MRP_XF_INVERTED) != 0;
        const uint32_t C1 = c.C1, C2 = c.C2, C = C1 * C2;
        const bool a_cells_paired = inv && c.a_part && c.d1 > 0, b_cells_paired = inv && c.b_part && c.d2 > 0;
        /* MRP_XF_UNITS: one array entry per complement pair (the even cell's cost, its transitions as merge UNIT indices) */
        const bool units = (c.flags & MRP_XF_UNITS) != 0;
        const uint32_t ush = units && (a_cells_paired || b_cells_paired) ? 1u : 0u; /* entry of cell e: e >> ush, written for even e */
        const uint32_t nsh = units && (c.flags & (MRP_XF_OUT_A_PAIRED | MRP_XF_OUT_B_PAIRED)) ? 1u : 0u;
        const uint32_t psh = units && (c.flags & (MRP_XF_IN_A_PAIRED | MRP_XF_IN_B_PAIRED)) ? 1u : 0u;
        auto np_entry = [&](uint32_t v) -> uint32_t { return ((v & 0xFFFFu) >> nsh) | (((v >> 16) >> psh) << 16); };
        /* slots per table fill: rows of the tables are padded to a multiple of four slots, the staging buffer holds XE_ROWS */
        const uint32_t Cs = C1 + C2;
        const uint32_t slot_room = (Cs >= 1u && Cs <= 256u) ? min((uint32_t) XE_ROWS, (cap / Cs) & ~3u) : 0u;
        const uint32_t A_uni = (dc.flags >> 8) & 0xFFu; /* allele count shared by the column's sites, 0 if they differ (layout kernel) */
        const int w4_all = (dc.depth + 15) >> 4;
        const int w4_a = ((int) c.d1 + 15) >> 4, w4_b = (int) c.d1 >> 4;
        /* narrow column: every array entry and every parent cell has a lane of its own */
        const bool narrow = (C >> ush) <= (uint32_t) WAVE && C1 <= (uint32_t) WAVE && C2 <= (uint32_t) WAVE;
        if (MODE == 1 ? !narrow : (MODE == 2 && narrow)) continue;
        if (MODE != 2 && narrow) {
            const bool have_a = c.a_part != nullptr, have_b = c.b_part != nullptr;
            const bool ia = have_a && (uint32_t) lane < C1, ib = have_b && (uint32_t) lane < C2;
            uint32_t npa[2] = {ia ? c.a_np[lane] : 0u, 0u}, npb[2] = {ib ? c.b_np[lane] : 0u, 0u};
            uint64_t Pa[2] = {ia ? c.a_part[lane] : 0ull, 0ull}, Pb[2] = {ib ? c.b_part[lane] : 0ull, 0ull};
            XE_T(1);
            int bad = xe_verify_side<1>(have_a, Pa, npa, C1, c.d1, c.Ma, c.Pa, c.out_a, c.in_a, inv,
                                        (c.flags & MRP_XF_OUT_A_PAIRED) != 0, (c.flags & MRP_XF_IN_A_PAIRED) != 0, lane);
            bad |= xe_verify_side<1>(have_b, Pb, npb, C2, c.d2, c.Mb, c.Pb, c.out_b, c.in_b, inv,
                                     (c.flags & MRP_XF_OUT_B_PAIRED) != 0, (c.flags & MRP_XF_IN_B_PAIRED) != 0, lane);
            if ((!c.a_part && C1 != 1u) || (!c.b_part && C2 != 1u) || (int) c.d1 + (int) c.d2 != dc.depth) bad |= MRP_ENGINE_ERR_RANGE;
            if (bad) { atomicOr(err, bad); atomicOr(err_hmm + col_hmm[col], bad); }
            const uint32_t U = C >> ush;
            if (__any(bad != 0)) { /* the level is discarded by the host; keep the arrays defined meanwhile */
                if ((uint32_t) lane < U) { cell_np[c.x_cell_off + lane] = 0u; cell_cost[c.x_cell_off + lane] = 0u; }
                continue;
            }
            /* the lane's cell, its parents' partitions and transitions (from the lanes that hold them) */
            uint32_t c1, c2;
            cross_cell(((uint32_t) lane < U ? (uint32_t) lane : 0u) << ush, C2, inv, a_cells_paired, b_cells_paired, c1, c2);
            const uint32_t n1 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c1 << 2), (int) npa[0]);
            const uint32_t n2 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c2 << 2), (int) npb[0]);
            const uint64_t p1 = ((uint64_t) (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c1 << 2), (int) (uint32_t) (Pa[0] >> 32)) << 32) |
                                (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c1 << 2), (int) (uint32_t) Pa[0]);
            const uint64_t p2 = ((uint64_t) (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c2 << 2), (int) (uint32_t) (Pb[0] >> 32)) << 32) |
                                (uint32_t) __builtin_amdgcn_ds_bpermute((int) (c2 << 2), (int) (uint32_t) Pb[0]);
            const uint64_t P = c.d1 < 64 ? (p1 | (p2 << c.d1)) : p1; /* mergePartitionsOrMasks, partitions.c:21-28 */
            const uint32_t npv = np_entry(cross_np(c, inv, c1, c2, n1, n2));
            XE_T(2);
            /* the sites in chunks of whole sites of at most 16 slots; `ends` marks the last allele slot of every site */
            const uint32_t *aoff = A_uni ? nullptr : chunks[dc.chunk].allele_offset + dc.site_start;
            uint32_t sel[16];
#pragma unroll
            for (int w = 0; w < 16; w++) sel[w] = ((uint32_t) ((P >> (4 * w)) & 0xFull) * 0x00204081u) & 0x01010101u;
            uint32_t cost = 0, site0 = 0, sl0 = 0, m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
            if (A_uni == 2u && 2u * U < 2u * (uint32_t) dc.n_sites) { /* few cells, many sites: lanes along the slots */
                const uint32_t n_slots = 2u * (uint32_t) dc.n_sites;
                for (uint32_t s0 = 0; s0 < n_slots; s0 += WAVE) {
                    const uint32_t nsl = min((uint32_t) WAVE, n_slots - s0);
                    const int64_t sg = dc.slot_off + s0;
                    switch (w4_all) {
                    case 0: case 1: cost += xe_slots_chunk<1>(slot_bytes, slot_total, sg, nsl, U, P, lane); break;
                    case 2: cost += xe_slots_chunk<2>(slot_bytes, slot_total, sg, nsl, U, P, lane); break;
                    case 3: cost += xe_slots_chunk<3>(slot_bytes, slot_total, sg, nsl, U, P, lane); break;
                    default: cost += xe_slots_chunk<4>(slot_bytes, slot_total, sg, nsl, U, P, lane); break;
                    }
                }
                site0 = (uint32_t) dc.n_sites;
            }
            while (site0 < (uint32_t) dc.n_sites) {
                uint32_t cnt, nsl, ends = 0;
                if (A_uni && A_uni <= 16u) {
                    cnt = min((uint32_t) dc.n_sites - site0, 16u / A_uni);
                    nsl = cnt * A_uni;
                    if (A_uni == 2u) ends = 0xAAAAu & ((1u << nsl) - 1u);
                    else for (uint32_t s_ = 1; s_ <= cnt; s_++) ends |= 1u << (s_ * A_uni - 1u);
                } else { /* lane s looks at the end of site site0 + s */
                    const uint32_t *ao = A_uni ? chunks[dc.chunk].allele_offset + dc.site_start : aoff;
                    const uint32_t base = ao[site0];
                    const bool have = site0 + (uint32_t) lane < (uint32_t) dc.n_sites;
                    const uint32_t end = have ? ao[site0 + lane + 1] - base : 0xFFFFFFFFu;
                    const bool fits = have && end <= 16u;
                    cnt = (uint32_t) __popcll(__ballot(fits));
                    nsl = cnt ? (uint32_t) __builtin_amdgcn_readlane((int) end, (int) cnt - 1) : 0u;
                    ends = (fits && end >= 1u) ? 1u << (end - 1u) : 0u;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) ends |= (uint32_t) __shfl_xor((int) ends, o, WAVE);
                    if (cnt == 0) { /* a site of more than 16 alleles: slot by slot, the site ends with its last slot */
                        cnt = 1u;
                        nsl = ao[site0 + 1] - base;
                        const int64_t sg = dc.slot_off + sl0;
                        for (uint32_t a_ = 0; a_ < nsl; a_++) {
                            const uint32_t t = slot_dot(slot_bytes + (sg + a_) * 16, P, 0, w4_all);
                            m1 = min(m1, t);
                            m2 = min(m2, slot_total[sg + a_] - t);
                        }
                        cost += m1 + m2; m1 = 0xFFFFFFFFu; m2 = 0xFFFFFFFFu;
                        site0 += 1u; sl0 += nsl;
                        continue;
                    }
                }
                nsl = (uint32_t) __builtin_amdgcn_readfirstlane((int) nsl); /* (wave-uniform by construction; said again for the compiler) */
                ends = (uint32_t) __builtin_amdgcn_readfirstlane((int) ends);
                const int64_t sg = dc.slot_off + sl0;
                switch (w4_all) {
                case 0: case 1: cost += xe_narrow_chunk<1>(slot_bytes, slot_total, sg, nsl, ends, sel, lane, m1, m2); break;
                case 2: cost += xe_narrow_chunk<2>(slot_bytes, slot_total, sg, nsl, ends, sel, lane, m1, m2); break;
                case 3: cost += xe_narrow_chunk<3>(slot_bytes, slot_total, sg, nsl, ends, sel, lane, m1, m2); break;
                default: cost += xe_narrow_chunk<4>(slot_bytes, slot_total, sg, nsl, ends, sel, lane, m1, m2); break;
                }
                site0 += cnt;
                sl0 += nsl;
            }
            XE_T(3);
            if ((uint32_t) lane < U) {
                cell_np[c.x_cell_off + lane] = npv;
                cell_cost[c.x_cell_off + lane] = cost;
            }
            XE_T(4);
            continue;
        }
        if constexpr (MODE != 1) {
        /* Everything the column needs from HBM is requested HERE, in one round trip behind the two descriptors: the parents'
         * transitions and partitions (parent cells lane and lane + 64 of either side stay in the lane's registers: the pair
         * order check, the transition terms and the table rows all start from them) and, when the column's sites share their
         * allele count (so that the first table fill's slots are known from the descriptor alone), that fill's packed bytes
         * and byte sums.  Round 2 asked for them one after the other (transitions, order check, packed bytes, partitions):
         * four dependent trips to memory per column, half of the kernel's time. */
        const bool have_a = c.a_part != nullptr, have_b = c.b_part != nullptr;
        uint32_t npa[2], npb[2];
        uint64_t Pa[2], Pb[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t i = (uint32_t) lane + (uint32_t) u * WAVE;
            const bool ia = have_a && i < C1, ib = have_b && i < C2;
            npa[u] = ia ? c.a_np[i] : 0u;
            Pa[u] = ia ? c.a_part[i] : 0ull;
            npb[u] = ib ? c.b_np[i] : 0u;
            Pb[u] = ib ? c.b_part[i] : 0ull;
        }
        constexpr int XE_PRE = XE_ROWS * 16 / WAVE;
        const uint32_t pre_cnt = A_uni ? min((uint32_t) dc.n_sites, slot_room / A_uni) : 0u;
        const uint32_t pre_nsl = pre_cnt * A_uni; /* 0: the first fill asks for its slots itself */
        uint32_t pre_rows[XE_PRE], pre_tot = 0u;
#pragma unroll
        for (int k = 0; k < XE_PRE; k++) {
            const uint32_t i = (uint32_t) lane + (uint32_t) k * WAVE;
            pre_rows[k] = i < pre_nsl * 16u ? slot_bytes[dc.slot_off * 16 + i] : 0u;
        }
        if ((uint32_t) lane < pre_nsl) pre_tot = slot_total[dc.slot_off + lane];
#ifdef XE_CLOCK
        if (__builtin_amdgcn_readfirstlane((int) (npa[0] ^ npb[0] ^ pre_rows[0] ^ (uint32_t) Pa[0] ^ (uint32_t) Pb[0])) == 0x7EADBEEF) continue; /* wait for the loads: section 1 */
        XE_T(1);
#endif
        xe_stage_transitions(c, inv, tra, trb, lane, npa, npb);
        int bad = xe_verify_side(have_a, Pa, npa, C1, c.d1, c.Ma, c.Pa, c.out_a, c.in_a, inv,
                                 (c.flags & MRP_XF_OUT_A_PAIRED) != 0, (c.flags & MRP_XF_IN_A_PAIRED) != 0, lane);
        bad |= xe_verify_side(have_b, Pb, npb, C2, c.d2, c.Mb, c.Pb, c.out_b, c.in_b, inv,
                              (c.flags & MRP_XF_OUT_B_PAIRED) != 0, (c.flags & MRP_XF_IN_B_PAIRED) != 0, lane);
        if ((!c.a_part && C1 != 1u) || (!c.b_part && C2 != 1u) || C1 > 128u || C2 > 128u || (int) c.d1 + (int) c.d2 != dc.depth) bad |= MRP_ENGINE_ERR_RANGE;
        if (bad) { atomicOr(err, bad); atomicOr(err_hmm + col_hmm[col], bad); }
        if (__any(bad != 0)) { /* the level is discarded by the host; keep the arrays defined meanwhile */
            for (uint32_t e = lane; e < (C >> ush); e += WAVE) { cell_np[c.x_cell_off + e] = 0u; cell_cost[c.x_cell_off + e] = 0u; }
            continue;
        }
        const uint32_t *aoff = A_uni ? nullptr : chunks[dc.chunk].allele_offset + dc.site_start;
        uint32_t site0 = 0, sl0 = 0;
        XE_T(2); /* transition terms, order check */
        /* one table fill and the cells' costs over its sites; the first is called with the registers above, the others (columns
         * of many sites or alleles: the low levels) ask again, so that nothing of the front end stays live over the cells */
        auto fill_and_cost = [&](const bool first_chunk, uint64_t Qa0, uint64_t Qa1, uint64_t Qb0, uint64_t Qb1) {
            /* as many whole sites as fit */
            uint32_t cnt, nsl;
            uint64_t ends = 0; /* bit (slot): the slot is the last allele of its site */
            if (A_uni) {
                cnt = min((uint32_t) dc.n_sites - site0, slot_room / A_uni);
                nsl = cnt * A_uni;
                for (uint32_t s_ = 1; s_ <= cnt; s_++) ends |= 1ull << (s_ * A_uni - 1u);
            } else { /* lane s looks at the end of site site0 + s */
                const uint32_t base = aoff[site0];
                const bool have = site0 + (uint32_t) lane < (uint32_t) dc.n_sites;
                const uint32_t end = have ? aoff[site0 + lane + 1] - base : 0xFFFFFFFFu;
                const bool fits = have && end <= slot_room;
                cnt = (uint32_t) __popcll(__ballot(fits));
                nsl = cnt ? (uint32_t) __builtin_amdgcn_readlane((int) end, (int) cnt - 1) : 0u;
                ends = (fits && end >= 1u) ? 1ull << (end - 1u) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) ends |= __shfl_xor(ends, o, WAVE);
                ends = ((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) (ends >> 32)) << 32) |
                       (uint32_t) __builtin_amdgcn_readfirstlane((int) ends); /* wave-uniform: the site loop branches on scalars */
            }
            const int64_t slot_g = dc.slot_off + sl0;
            if (cnt == 0) {
                /* A site with more alleles than the tables hold for this many parent cells (rare): its cells are costed
                 * one by one from their merged partitions, straight from the packed bytes in HBM. */
                const uint32_t A = A_uni ? A_uni : aoff[site0 + 1] - aoff[site0];
                for (uint32_t en = lane; en < (C >> ush); en += WAVE) {
                    const uint32_t e = en << ush;
                    uint32_t c1, c2;
                    cross_cell(e, C2, inv, a_cells_paired, b_cells_paired, c1, c2);
                    const uint64_t P = cross_partition(c, c1, c2);
                    uint32_t m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
                    for (uint32_t a_ = 0; a_ < A; a_++) {
                        const uint32_t t = slot_dot(slot_bytes + (slot_g + a_) * 16, P, 0, w4_all);
                        m1 = min(m1, t);
                        m2 = min(m2, slot_total[slot_g + a_] - t);
                    }
                    const int64_t o = c.x_cell_off + en;
                    if (first_chunk) {
                        cell_np[o] = np_entry(xe_np(tra[c1], trb[c2]));
                        cell_cost[o] = m1 + m2;
                    } else cell_cost[o] += m1 + m2;
                }
                site0 += 1u;
                sl0 += A;
                return;
            }
            const uint32_t ST = (nsl + 3u) & ~3u; /* row stride: 16-byte rows */
            uint32_t *tb = tab + C1 * ST;
            {
                /* the packed bytes and byte sums of the slots: one coalesced read (the first fill's is in flight since the top of
                 * the column), then LDS */
                if (first_chunk && pre_nsl) {
#pragma unroll
                    for (int k = 0; k < XE_PRE; k++) {
                        const uint32_t i = (uint32_t) lane + (uint32_t) k * WAVE;
                        if (i < nsl * 16u) rowbuf[i] = pre_rows[k];
                    }
                    if ((uint32_t) lane < nsl) totbuf[lane] = pre_tot;
                } else {
                    for (uint32_t i = lane; i < nsl * 16u; i += WAVE) rowbuf[i] = slot_bytes[slot_g * 16 + i];
                    if ((uint32_t) lane < nsl) totbuf[lane] = slot_total[slot_g + lane];
                }
                wave_lds_fence();
                if (Cs >= 24u) { /* many parent cells: a lane per parent cell */
                    const uint32_t *rowb = rowbuf + 4 * w4_b;
                    switch (w4_a) {
                    case 0: case 1: xe_fill_side<1, false>(tab, ST, Qa0, Qa1, C1, 0u, 0u, nsl, rowbuf, totbuf, lane); break;
                    case 2: xe_fill_side<2, false>(tab, ST, Qa0, Qa1, C1, 0u, 0u, nsl, rowbuf, totbuf, lane); break;
                    case 3: xe_fill_side<3, false>(tab, ST, Qa0, Qa1, C1, 0u, 0u, nsl, rowbuf, totbuf, lane); break;
                    default: xe_fill_side<4, false>(tab, ST, Qa0, Qa1, C1, 0u, 0u, nsl, rowbuf, totbuf, lane); break;
                    }
                    switch (min(w4_all, 4) - min(w4_b, 3)) { /* d1 = 64: side B has no reads, any group of zero bits will do */
                    case 0: case 1: xe_fill_side<1, true>(tb, ST, Qb0, Qb1, C2, c.d1, 16u * min(w4_b, 3), nsl, rowbuf + 4 * min(w4_b, 3), totbuf, lane); break;
                    case 2: xe_fill_side<2, true>(tb, ST, Qb0, Qb1, C2, c.d1, 16u * w4_b, nsl, rowb, totbuf, lane); break;
                    case 3: xe_fill_side<3, true>(tb, ST, Qb0, Qb1, C2, c.d1, 16u * w4_b, nsl, rowb, totbuf, lane); break;
                    default: xe_fill_side<4, true>(tb, ST, Qb0, Qb1, C2, c.d1, 16u * w4_b, nsl, rowb, totbuf, lane); break;
                    }
                } else { /* few parent cells (the low levels: long columns of few cells): lanes along (slot, parent cell); the
                          * partition of parent cell cc comes from lane cc's register */
                    for (uint32_t i0 = 0; i0 < C1 * nsl; i0 += WAVE) {
                        const uint32_t idx = i0 + (uint32_t) lane;
                        const bool act = idx < C1 * nsl;
                        const uint32_t slot = act ? idx / C1 : 0u, cc = act ? idx - slot * C1 : 0u;
                        const uint64_t P = ((uint64_t) (uint32_t) __shfl((int) (uint32_t) (Qa0 >> 32), (int) cc, WAVE) << 32) |
                                           (uint32_t) __shfl((int) (uint32_t) Qa0, (int) cc, WAVE);
                        if (act) {
                            const uint32_t t = slot_dot(rowbuf + slot * 16, P, 0, w4_a);
                            tab[cc * ST + slot] = t | ((totbuf[slot] - t) << 16);
                        }
                    }
                    for (uint32_t i0 = 0; i0 < C2 * nsl; i0 += WAVE) {
                        const uint32_t idx = i0 + (uint32_t) lane;
                        const bool act = idx < C2 * nsl;
                        const uint32_t slot = act ? idx / C2 : 0u, cc = act ? idx - slot * C2 : 0u;
                        const uint64_t Pr = ((uint64_t) (uint32_t) __shfl((int) (uint32_t) (Qb0 >> 32), (int) cc, WAVE) << 32) |
                                            (uint32_t) __shfl((int) (uint32_t) Qb0, (int) cc, WAVE);
                        if (act) {
                            const uint64_t P = c.d1 < 64 ? Pr << c.d1 : 0ull;
                            const uint32_t t = slot_dot(rowbuf + slot * 16, P, w4_b, w4_all);
                            tb[cc * ST + slot] = t - (t << 16);
                        }
                    }
                }
            }
            /* biallelic sites, unit level (the shipped ONT parameters: every level above the first): the cells' loop below takes the
             * slots four at a time without looking at `ends`; the rows' padding up to a multiple of four slots is zeroed (a pad pair
             * then costs 0 + 0) */
            const bool fast2 = units && a_cells_paired && A_uni == 2u;
            if (fast2 && ST > nsl)
                for (uint32_t i = lane; i < Cs; i += WAVE) {
                    uint32_t *rw = tab + i * ST; /* (side B's rows follow side A's: tb = tab + C1 * ST) */
                    for (uint32_t s_ = nsl; s_ < ST; s_++) rw[s_] = 0u;
                }
            wave_lds_fence();
            XE_T(3); /* table fill */
            if (fast2) {
                /* the grid walk of the general branch below -- row r = pair (2r, 2r + 1) of side A cells, lane = side B cell h -- with
                 * everything that does not depend on the row hoisted: the lane's table row (up to 16 slots in registers), its two
                 * transition terms per direction, and the store addresses, which advance by a constant.  Per unit: an add and half a
                 * packed min per slot, two adds per site, seven operations for the transitions. */
                const uint32_t W = C2 >= 33u ? 64u : (C2 >= 17u ? 32u : (C2 >= 9u ? 16u : (C2 >= 5u ? 8u : (C2 >= 3u ? 4u : (C2 >= 2u ? 2u : 1u)))));
                const uint32_t wsh = 31u - (uint32_t) __builtin_clz(W), R = WAVE >> wsh;
                const uint32_t hl = (uint32_t) lane & (W - 1u), rl = (uint32_t) lane >> wsh, rows = C1 >> 1;
                const uint32_t nq = ST >> 2;
                for (uint32_t hb = 0; hb < C2; hb += WAVE) {
                    const uint32_t h = hb + hl;
                    const bool hv = h < C2;
                    const uint32_t hc = hv ? h : 0u;
                    const uint2 tbh = trb[hc];
                    const uint32_t bn_lo = tbh.x & 0xFFFFu, bn_hi = tbh.x >> 16, bp_lo = tbh.y & 0xFFFFu, bp_hi = tbh.y >> 16;
                    const uint32_t *pb = tb + hc * ST;
                    uint4 bq[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) bq[q] = (uint32_t) q < nq ? *reinterpret_cast<const uint4 *>(pb + 4 * q) : make_uint4(0, 0, 0, 0);
                    uint32_t *pn = cell_np + c.x_cell_off + ((int64_t) rl * C2 + h), *pc = cell_cost + c.x_cell_off + ((int64_t) rl * C2 + h);
                    const uint32_t stride = R * C2;
                    /* two rows per step (r and r + R), their table rows and transition terms requested together; NQ = groups of four
                     * slots, a compile-time constant per instantiation: the body is straight-line code */
                    auto walk = [&](auto nq_tag) {
                        constexpr int NQ = decltype(nq_tag)::value;
                        constexpr bool TWO = NQ <= 2; /* (two rows of 12 or 16 slots in flight cost the fifth wave per SIMD its registers) */
                        for (uint32_t r = rl; r < rows; r += (TWO ? 2u : 1u) * R) {
                            const uint32_t r2 = r + R;
                            const bool v2 = TWO && r2 < rows;
                            const uint32_t r2c = v2 ? r2 : r;
                            const uint32_t *pa0 = tab + 2u * r * ST, *pa1 = tab + 2u * r2c * ST;
                            uint4 a0[NQ], a1[TWO ? NQ : 1];
#pragma unroll
                            for (int q = 0; q < NQ; q++) { a0[q] = *reinterpret_cast<const uint4 *>(pa0 + 4 * q); if (TWO) a1[q] = *reinterpret_cast<const uint4 *>(pa1 + 4 * q); }
                            const uint2 ta0 = tra[2u * r], ta1 = TWO ? tra[2u * r2c] : make_uint2(0u, 0u);
                            uint32_t cost0 = 0, cost1 = 0;
#pragma unroll
                            for (int q = 0; q < NQ; q++) {
                                const uint32_t m01 = pk_min_u16(a0[q].x + bq[q].x, a0[q].y + bq[q].y), m23 = pk_min_u16(a0[q].z + bq[q].z, a0[q].w + bq[q].w);
                                cost0 += (m01 & 0xFFFFu) + (m01 >> 16) + (m23 & 0xFFFFu) + (m23 >> 16);
                                if (TWO) {
                                    const uint32_t n01 = pk_min_u16(a1[q].x + bq[q].x, a1[q].y + bq[q].y), n23 = pk_min_u16(a1[q].z + bq[q].z, a1[q].w + bq[q].w);
                                    cost1 += (n01 & 0xFFFFu) + (n01 >> 16) + (n23 & 0xFFFFu) + (n23 >> 16);
                                }
                            }
                            const uint32_t nx0 = (ta0.x & 0x7FFFFFFFu) + ((int32_t) ta0.x < 0 ? bn_hi : bn_lo), pv0 = (ta0.y & 0x7FFFFFFFu) + ((int32_t) ta0.y < 0 ? bp_hi : bp_lo);
                            const uint32_t nx1 = (ta1.x & 0x7FFFFFFFu) + ((int32_t) ta1.x < 0 ? bn_hi : bn_lo), pv1 = (ta1.y & 0x7FFFFFFFu) + ((int32_t) ta1.y < 0 ? bp_hi : bp_lo);
                            if (hv) {
                                if (first_chunk) { pn[0] = (nx0 >> nsh) | ((pv0 >> psh) << 16); if (v2) pn[stride] = (nx1 >> nsh) | ((pv1 >> psh) << 16); }
                                else { cost0 += pc[0]; if (v2) cost1 += pc[stride]; }
                                pc[0] = cost0;
                                if (v2) pc[stride] = cost1;
                            }
                            pn += (TWO ? 2u : 1u) * stride; pc += (TWO ? 2u : 1u) * stride;
                        }
                    };
                    switch (nq) {
                    case 1: walk(std::integral_constant<int, 1>()); break;
                    case 2: walk(std::integral_constant<int, 2>()); break;
                    case 3: walk(std::integral_constant<int, 3>()); break;
                    default: walk(std::integral_constant<int, 4>()); break;
                    }
                }
            } else if (a_cells_paired) {
                /* The cells of the column are a grid: row r = pair (2r, 2r + 1) of side A cells, position h = side B cell;
                 * cells e = 2 (r C2 + h) and e + 1 are complements and share their cost.  A lane keeps ONE h: its side B
                 * table row and transition terms stay in registers while it walks down the rows; with C2 <= 32 a wave
                 * takes several rows per step.  Per cell that leaves an add and a packed min per allele slot. */
                const uint32_t W = C2 >= 33u ? 64u : (C2 >= 17u ? 32u : (C2 >= 9u ? 16u : (C2 >= 5u ? 8u : (C2 >= 3u ? 4u : (C2 >= 2u ? 2u : 1u)))));
                const uint32_t wsh = 31u - (uint32_t) __builtin_clz(W), R = WAVE >> wsh;
                const uint32_t hl = (uint32_t) lane & (W - 1u), rl = (uint32_t) lane >> wsh, rows = C1 >> 1;
                for (uint32_t hb = 0; hb < C2; hb += WAVE) {
                    const uint32_t h = hb + hl;
                    const bool hv = h < C2;
                    const uint32_t hc = hv ? h : 0u, g = b_cells_paired ? (hc ^ 1u) : hc;
                    const uint2 tbh = trb[hc], tbg = trb[g];
                    const uint32_t *pb = tb + hc * ST;
                    uint4 b0 = make_uint4(0, 0, 0, 0), b1 = make_uint4(0, 0, 0, 0);
                    if (nsl <= 8u) { b0 = *reinterpret_cast<const uint4 *>(pb); if (nsl > 4u) b1 = *reinterpret_cast<const uint4 *>(pb + 4); }
                    for (uint32_t r = rl; r < rows; r += R) {
                        const uint32_t *pa = tab + 2u * r * ST;
                        uint32_t cost;
                        if (nsl <= 8u) {
                            uint32_t m = 0xFFFFFFFFu;
                            cost = 0;
                            const uint4 a0 = *reinterpret_cast<const uint4 *>(pa);
                            const uint32_t x0[4] = {a0.x + b0.x, a0.y + b0.y, a0.z + b0.z, a0.w + b0.w};
#pragma unroll
                            for (int j = 0; j < 4; j++)
                                if ((uint32_t) j < nsl) {
                                    m = pk_min_u16(m, x0[j]);
                                    if (ends & (1ull << j)) { cost += (m & 0xFFFFu) + (m >> 16); m = 0xFFFFFFFFu; }
                                }
                            if (nsl > 4u) {
                                const uint4 a1 = *reinterpret_cast<const uint4 *>(pa + 4);
                                const uint32_t x1[4] = {a1.x + b1.x, a1.y + b1.y, a1.z + b1.z, a1.w + b1.w};
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    if ((uint32_t) (4 + j) < nsl) {
                                        m = pk_min_u16(m, x1[j]);
                                        if (ends & (1ull << (4 + j))) { cost += (m & 0xFFFFu) + (m >> 16); m = 0xFFFFFFFFu; }
                                    }
                            }
                        } else cost = xe_cost(pa, pb, nsl, ends);
                        if (hv && units) { /* one entry per pair: a dword per lane and array, lanes along h */
                            const int64_t o = c.x_cell_off + ((int64_t) r * C2 + h);
                            if (first_chunk) cell_np[o] = np_entry(xe_np(tra[2u * r], tbh));
                            else cost += cell_cost[o];
                            cell_cost[o] = cost;
                        } else if (hv) {
                            const int64_t o = c.x_cell_off + 2 * ((int64_t) r * C2 + h);
                            if (first_chunk) {
                                const uint4 ta = *reinterpret_cast<const uint4 *>(tra + 2u * r); /* terms of cells 2r and 2r + 1 */
                                xe_u32x2 nv = {xe_np(make_uint2(ta.x, ta.y), tbh), xe_np(make_uint2(ta.z, ta.w), tbg)};
                                *reinterpret_cast<xe_u32x2 *>(cell_np + o) = nv;
                            } else cost += cell_cost[o];
                            xe_u32x2 cv = {cost, cost};
                            *reinterpret_cast<xe_u32x2 *>(cell_cost + o) = cv;
                        }
                    }
                }
            } else {
                for (uint32_t en = lane; en < (C >> ush); en += WAVE) {
                    const uint32_t e = en << ush;
                    uint32_t c1, c2;
                    cross_cell(e, C2, inv, a_cells_paired, b_cells_paired, c1, c2);
                    const uint32_t cost = xe_cost(tab + c1 * ST, tb + c2 * ST, nsl, ends);
                    const int64_t o = c.x_cell_off + en;
                    if (first_chunk) {
                        cell_np[o] = np_entry(xe_np(tra[c1], trb[c2]));
                        cell_cost[o] = cost;
                    } else cell_cost[o] += cost;
                }
            }
            wave_lds_fence(); /* the tables are rewritten by the next chunk of sites / the next column */
            XE_T(4); /* cells */
            site0 += cnt;
            sl0 += nsl;
        };
        if ((uint32_t) dc.n_sites > 0u) fill_and_cost(true, Pa[0], Pa[1], Pb[0], Pb[1]);
        while (site0 < (uint32_t) dc.n_sites) {
            uint64_t Qa[2], Qb[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint32_t i = (uint32_t) lane + (uint32_t) u * WAVE;
                Qa[u] = (have_a && i < C1) ? c.a_part[i] : 0ull;
                Qb[u] = (have_b && i < C2) ? c.b_part[i] : 0ull;
            }
            fill_and_cost(false, Qa[0], Qa[1], Qb[0], Qb[1]);
        }
        } /* MODE != 1 */
    }
#ifdef XE_CLOCK
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    XE_T(5); /* the stores in flight at the end */
    if (lane == 0 && (blockIdx.x & 63u) == 0u) for (int i = 0; i < 8; i++) atomicAdd((unsigned long long *) (err + 4) + i, (unsigned long long) xe_sec[i]); /* a sample of the waves */
#endif
}

hipError_t mrp_launch_cross_emit(const CrossCol *cols_dev, const MrpBatchDev &d, int32_t *err, const int32_t *col_hmm_dev, int32_t *err_hmm,
                                 int32_t level_max_cells, bool mostly_narrow, hipStream_t stream, LaunchCensus *census) {
    if (d.n_cols <= 0) return hipSuccess;
    int64_t wgs = (d.n_cols + XE_WAVES - 1) / XE_WAVES;
    const CrossEmitPlan plan = cross_emit_plan(level_max_cells, mostly_narrow); /* (mrp_level_order.h) */
    if (census) census->bump(plan.census_slot);
    const uint32_t cap = plan.wide_cap ? XE_CAP_WIDE : XE_CAP_NARROW;
    const size_t lds = (size_t) XE_WAVES * (cap + XE_ROWS * 16 + XE_ROWS + 512) * sizeof(uint32_t);
    const dim3 grid((unsigned) (wgs < (1 << 20) ? wgs : (1 << 20)));
    if (plan.mode1) {
        hipLaunchKernelGGL(mrp_cross_emit_kernel<1>, grid, dim3(XE_WAVES * WAVE), 0, stream, cols_dev, d.cols, d.chunks, d.n_cols, d.slot_bytes, d.slot_total,
                           const_cast<uint32_t *>(d.cell_np), d.cell_cost, err, col_hmm_dev, err_hmm, cap);
        if (plan.mode2)
            hipLaunchKernelGGL(mrp_cross_emit_kernel<2>, grid, dim3(XE_WAVES * WAVE), lds, stream, cols_dev, d.cols, d.chunks, d.n_cols, d.slot_bytes, d.slot_total,
                               const_cast<uint32_t *>(d.cell_np), d.cell_cost, err, col_hmm_dev, err_hmm, cap);
    } else
        hipLaunchKernelGGL(mrp_cross_emit_kernel<0>, grid, dim3(XE_WAVES * WAVE), lds, stream, cols_dev, d.cols, d.chunks, d.n_cols, d.slot_bytes, d.slot_total,
                           const_cast<uint32_t *>(d.cell_np), d.cell_cost, err, col_hmm_dev, err_hmm, cap);
    return hipGetLastError();
}
