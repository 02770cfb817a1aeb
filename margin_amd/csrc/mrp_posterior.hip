/*
 * mrp_posterior.hip -- the posterior half of the banded pairwise aligner: getPosteriorProbsWithBanding
 * (impl/pairwiseAligner.c:706-844) with diagonalCalculationPosteriorMatchProbs (:610-635) or diagonalCalculationPosteriorProbs
 * (:637-681) for batches of string pairs.  gfx950 only; compiled with -ffp-contract=off.  DESIGN.md 9.15.
 *
 * The reference walks a pair's band forward and, at the diagonals the band alone decides (mrp_posterior_plan.h), walks a stretch of it
 * back.  Once the forward diagonals exist the tracebacks do not depend on one another, so the device runs them side by side:
 *
 *   pst_forward_kernel     a pair per wave: the forward walk of mrp_pairhmm_walk.h, which here also stores every band cell's three
 *                          states into the pair's slice of a workspace, an array per state.
 *   pst_traceback_kernel   a (pair, traceback) per wave: three backward diagonals rotate in LDS, the forward ones are read from the
 *                          workspace; a lane gathers a cell from its three successors (pst_backward_cell, same header).  The totals
 *                          (:578-596) are folded by one lane in index order.  Cells whose log posterior reaches a cut the host put a
 *                          little below log(threshold) are compacted, by ballot, into space sized from the plan.
 *   pst_pack_kernel        moves the candidates of the tracebacks behind one another: what is downloaded is 16 B per candidate.
 *   pst_forward_wide_kernel, pst_traceback_wide_kernel
 *                          the same with a workgroup per pair / per (pair, traceback), for the pairs whose widest diagonal exceeds
 *                          the 2 048 cells the LDS of the two above holds (mrp_context_set_posterior_wide_pairs).
 *
 * The band is the host's, (l, r) per diagonal: band_construct's for mrp_posterior_aligned_pairs, band_constructDynamic's for
 * mrp_posterior_aligned_pairs_dynamic (mrp_band.h); the kernels do not know which.
 *
 * In the pair-per-wave kernels a workgroup is one wave and what it hands from step to step lives in LDS, so the barrier between steps is
 * lds_barrier(), which orders LDS traffic only: nothing in them reads what it stored to the workspace or to the lists.
 *
 * The host applies the reference's rule (addPosteriorProb, :598-608) with the C library's exp and keeps the order of generation.
 *
 * The four walking kernels are templates over the match emission (mrp_pairhmm_walk.h): mrp_posterior_aligned_pairs_rle runs their
 * PhmRunLength instantiations over the same plan, groups and lists.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_band.h"
#include "mrp_internal.h"
#include "mrp_pairhmm.h"
#include "mrp_pairhmm_walk.h" /* the forward walk and the cells of a traceback; PstPair, PstTb */
#include "mrp_posterior_plan.h"
#include "mrp_wave.h" /* lds_barrier */

#pragma clang fp contract(off)

namespace {

constexpr int64_t PST_DEFAULT_WORKSPACE = (int64_t) MRP_POSTERIOR_DEFAULT_WORKSPACE;
constexpr int64_t PST_CELL_BYTES = 24; /* three states of a band cell */

struct PstCand {
    int32_t x, y; /* sequence coordinates, -1 for the gap before the first symbol */
    double v;     /* the log posterior whose exp() the host tests */
};
static_assert(sizeof(PstCand) == 16, "a candidate is 16 bytes");

/* A pair per wave: the walk with the live diagonals in LDS (3 diagonals x W cells x 3 states) and every cell kept,
 * ws_m / ws_x / ws_y [cell_first[diag0 + d] + i] = cell i of diagonal d.  Nothing here reads what it stored to the workspace. */
template <class Em>
__global__ void __launch_bounds__(PHM_WAVE) pst_forward_kernel(const PstPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                                 const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band,
                                                                 const int64_t *__restrict__ cell_first, int W, double *__restrict__ ws_m,
                                                                 double *__restrict__ ws_x, double *__restrict__ ws_y, typename Em::Args ea) {
    extern __shared__ double pst_lds[];
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PstPair p = pairs[pi];
        const PhmPairCtxT<Em> c = phm_pair_ctx<Em>(models, p.model, pool, p.x_off, p.y_off, ea);
        PhmDiagonals<PhmInterleaved, PHM_KEEP_ALSO> diag{PhmInterleaved::at(pst_lds, W, 0), PhmInterleaved::at(pst_lds, W, 1), PhmInterleaved::at(pst_lds, W, 2), {ws_m, ws_x, ws_y, cell_first + p.diag0}};
        phm_forward_walk<PhmTeam<PHM_WAVE, true>>(p.lx + p.ly, diag, PhmBandLimits{band + 2 * p.diag0}, c);
    }
}

/* Appends the cells of a diagonal that keep (lane by lane) to a traceback's list, in index order: ballot, rank among the lanes below */
static __device__ __forceinline__ void pst_emit(PstCand *__restrict__ list, int &count, bool keep, int x, int y, double v) {
    const unsigned long long mask = __ballot(keep);
    if (keep) {
        const int rank = __popcll(mask & ((1ull << threadIdx.x) - 1ull));
        list[count + rank] = PstCand{x, y, v};
    }
    count += __popcll(mask);
}

/* One traceback of one pair (pairwiseAligner.c:752-829), a wave.  b0 / b1 / b2: the backward diagonals d', d' + 1, d' + 2, each gathered
 * from the two behind it (pst_backward_cell, which says in what order). */
template <class Em>
__global__ void __launch_bounds__(PHM_WAVE) pst_traceback_kernel(const PstPair *__restrict__ pairs, const PstTb *__restrict__ tbs,
                                                                   const uint8_t *__restrict__ pool, const PhmModelDev *__restrict__ models,
                                                                   const int32_t *__restrict__ band, const int64_t *__restrict__ cell_first, int W,
                                                                   const double *__restrict__ ws_m, const double *__restrict__ ws_x,
                                                                   const double *__restrict__ ws_y, double cut, int with_gaps, int ragged_right,
                                                                   int64_t n_tb_group, PstCand *__restrict__ cand_m, PstCand *__restrict__ cand_x,
                                                                   PstCand *__restrict__ cand_y, int32_t *__restrict__ counts,
                                                                   double *__restrict__ total_out, typename Em::Args ea) {
    extern __shared__ double pst_lds[]; /* 3 diagonals x W cells x 3 states */
    const int lane = threadIdx.x;
    const PstTb tb = tbs[blockIdx.x];
    const PstTbStartT<Em> s = pst_tb_start<Em>(tb, pairs, models, pool, band, cell_first, ragged_right, ea);
    const int d = tb.d;
    using View = PhmInterleaved;
    View b0 = View::at(pst_lds, W, 0), b1 = View::at(pst_lds, W, 1), b2 = View::at(pst_lds, W, 2);
    int l1 = 1, r1 = 0, l2 = 1, r2 = 0; /* the limits of d' + 1 and d' + 2: empty beyond d */
    PstCand *__restrict__ list_m = cand_m + tb.cand_base;
    PstCand *__restrict__ list_x = with_gaps ? cand_x + tb.cand_base : nullptr;
    PstCand *__restrict__ list_y = with_gaps ? cand_y + tb.cand_base : nullptr;
    int n_m = 0, n_x = 0, n_y = 0;
    int taken = 0; /* totalPosteriorCalculationsThisTraceback */
    double total = PHM_NEG;
    for (int dd = d; dd > tb.to; dd--) {
        const int l0 = s.bnd[2 * dd], r0 = s.bnd[2 * dd + 1];
        const int width = (r0 - l0) / 2 + 1;
        if (dd == d) {
            for (int i = lane; i < width; i += PHM_WAVE) b0.store(i, St{s.e_end[0], s.e_end[1], s.e_end[2]});
        } else {
            for (int i = lane; i < width; i += PHM_WAVE) b0.store(i, pst_backward_cell(dd, l0 + 2 * i, l1, r1, l2, r2, b1, b2, s.c));
        }
        lds_barrier();
        if (dd <= tb.from) {
            const PhmPlanarT<const double> fwd{ws_m, ws_x, ws_y, s.first[dd]};
            if (taken % 10 == 0) {
                /* diagonalCalculationTotalProbability (:578-596).  b2 is dead from here until the next diagonal is written into it:
                 * its first W doubles take the cells' terms of the first dot product, the next W those of the second */
                double *term = pst_lds + b2.first;
                for (int i = lane; i < width; i += PHM_WAVE) term[i] = pst_total_term_here(fwd.load(i), b0.load(i));
                const bool second = dd < d; /* diagonal dd + 1 has a backward diagonal; the forward diagonal dd - 1 always exists */
                const int width1 = second ? (r1 - l1) / 2 + 1 : 0;
                if (second) {
                    const int lm = s.bnd[2 * (dd - 1)], rm = s.bnd[2 * (dd - 1) + 1];
                    const PhmPlanarT<const double> fwd_m{ws_m, ws_x, ws_y, s.first[dd - 1]};
                    for (int j = lane; j < width1; j += PHM_WAVE)
                        term[W + j] = pst_total_term_next(dd, l1 + 2 * j, lm, rm, fwd_m, b1.load(j), s.c);
                }
                lds_barrier();
                if (lane == 0) {
                    /* dpDiagonal_dotProduct (:450-461): serially, ascending in x - y; phm_log_add is not associative */
                    double tot = PHM_NEG;
                    for (int i = 0; i < width; i++) tot = phm_log_add(tot, term[i]);
                    if (second) {
                        double tot1 = PHM_NEG;
                        for (int j = 0; j < width1; j++) tot1 = phm_log_add(tot1, term[W + j]);
                        tot = phm_log_add(tot, tot1);
                    }
                    term[2 * W] = tot;
                    if (dd == s.n) total_out[s.slot] = tot;
                }
                lds_barrier();
                total = term[2 * W];
            }
            taken++;
            /* diagonalCalculationPosteriorMatchProbs / ...PosteriorProbs (:610-681), ascending in x - y */
            for (int c0 = 0; c0 < width; c0 += PHM_WAVE) {
                const bool in = c0 + lane < width;
                const int i = in ? c0 + lane : 0;
                const int z = l0 + 2 * i;
                const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                double v;
                bool keep = pst_candidate(0, in, x, y, fwd.load(i).m, b0.load(i).m, total, cut, v);
                pst_emit(list_m, n_m, keep, x - 1, y - 1, v);
                if (with_gaps) {
                    keep = pst_candidate(1, in, x, y, fwd.load(i).x, b0.load(i).x, total, cut, v);
                    pst_emit(list_x, n_x, keep, x - 1, y - 1, v);
                    keep = pst_candidate(2, in, x, y, fwd.load(i).y, b0.load(i).y, total, cut, v);
                    pst_emit(list_y, n_y, keep, x - 1, y - 1, v);
                }
            }
        }
        lds_barrier(); /* every read of b2 (the terms, the total) is done before it is written as the next b0 */
        const View tmp = b2;
        b2 = b1; b1 = b0; b0 = tmp;
        l2 = l1; r2 = r1; l1 = l0; r1 = r0;
    }
    if (lane == 0) {
        counts[tb.slot] = n_m;
        counts[n_tb_group + tb.slot] = n_x;
        counts[2 * n_tb_group + tb.slot] = n_y;
    }
}

/* ---- pairs whose widest diagonal does not fit the LDS of the two kernels above (mrp_context_set_posterior_wide_pairs) ----------------
 * The same two walks with a WORKGROUP where the kernels above have a wave: the threads stride over a diagonal's cells, a cell's value
 * does not depend on which thread computes it, and what a step hands to the next lies in device memory.  A workgroup reads only what
 * it wrote itself and runs on one CU, whose waves share one vector L1: one __syncthreads() between the steps is the only
 * synchronisation, for the reason given above phm_wide_kernel.  The pointers that are read and written are not __restrict__. */

/* pst_forward_kernel with a pair per workgroup.  Every band cell is stored to the pair's slice of ws_m / ws_x / ws_y anyway, so the
 * diagonals d - 1 and d - 2 are read back from there: no copy in LDS, no second slice. */
template <int T, class Em>
__global__ void __launch_bounds__(T) pst_forward_wide_kernel(const PstPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                             const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band,
                                                             const int64_t *__restrict__ cell_first, double *ws_m, double *ws_x, double *ws_y,
                                                             typename Em::Args ea) {
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PstPair p = pairs[pi];
        const PhmPairCtxT<Em> c = phm_pair_ctx<Em>(models, p.model, pool, p.x_off, p.y_off, ea);
        PhmDiagonals<PhmPlanar, PHM_KEEP_ONLY> diag{{}, {}, {}, {ws_m, ws_x, ws_y, cell_first + p.diag0}};
        phm_forward_walk<PhmTeam<T, false>>(p.lx + p.ly, diag, PhmBandLimits{band + 2 * p.diag0}, c);
    }
}

/* pst_traceback_kernel with a (pair, traceback) per workgroup, grid-stride over the launch's tracebacks.  The workgroup's slice of a
 * second workspace, 11 * W doubles (W: the widest diagonal of the launch): the backward diagonals d', d' + 1, d' + 2 as
 * [diagonal][state][W], rotating by pointer, and the two rows of the total's terms.  The cell arithmetic is
 * pst_traceback_kernel's (mrp_pairhmm_walk.h).  The totals are folded serially, ascending in x - y, by the first wave (below).
 *   The candidates of a diagonal reach their lists ascending in x - y: the diagonal is walked in chunks of T cells, a wave takes a
 * ballot per list, lane 0 puts the wave's count into LDS, and behind one barrier a thread's slot is the list's running count + the
 * counts of the waves below + its rank in the ballot.  The counts are double buffered (a chunk's are read before the barrier of the
 * next chunk, written again behind it), so a chunk costs one barrier. */
/* One row of a total's terms folded in index order by a whole wave: it loads 64 terms at a time, and every lane adds them in the same
 * order, one lane's term after the other (v_readlane), so the chain is the serial one and no step of it waits for a load of its own */
static __device__ __forceinline__ double pst_fold_row(const double *row, int count, int lane) {
    double acc = PHM_NEG;
    for (int c0 = 0; c0 < count; c0 += PHM_WAVE) {
        const unsigned long long mine = (unsigned long long) __double_as_longlong(c0 + lane < count ? row[c0 + lane] : PHM_NEG);
        const int here = count - c0 < PHM_WAVE ? count - c0 : PHM_WAVE;
        for (int j = 0; j < here; j++) {
            const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) mine, j);
            const unsigned hi = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) (mine >> 32), j);
            acc = phm_log_add(acc, __longlong_as_double((long long) (((unsigned long long) hi << 32) | lo)));
        }
    }
    return acc;
}

template <int T, class Em>
__global__ void __launch_bounds__(T) pst_traceback_wide_kernel(const PstPair *__restrict__ pairs, const PstTb *__restrict__ tbs, int64_t n_tbs,
                                                               const uint8_t *__restrict__ pool, const PhmModelDev *__restrict__ models,
                                                               const int32_t *__restrict__ band, const int64_t *__restrict__ cell_first, int W,
                                                               const double *__restrict__ ws_m, const double *__restrict__ ws_x,
                                                               const double *__restrict__ ws_y, double *ws_back, double cut, int with_gaps,
                                                               int ragged_right, int64_t n_tb_group, PstCand *__restrict__ cand_m,
                                                               PstCand *__restrict__ cand_x, PstCand *__restrict__ cand_y,
                                                               int32_t *__restrict__ counts, double *__restrict__ total_out, typename Em::Args ea) {
    constexpr int NW = T / PHM_WAVE;
    static_assert(NW >= 2, "the two rows of a total are folded by two waves");
    __shared__ int wave_count[2][3][NW];
    __shared__ double row_total[2];
    const int tid = threadIdx.x, lane = tid & (PHM_WAVE - 1), wave = tid / PHM_WAVE;
    double *slice = ws_back + (size_t) blockIdx.x * 11 * (size_t) W;
    double *term = slice + 9 * (size_t) W;
    int flip = 0;
    for (int64_t k = blockIdx.x; k < n_tbs; k += gridDim.x) {
        const PstTb tb = tbs[k];
        const PstTbStartT<Em> s = pst_tb_start<Em>(tb, pairs, models, pool, band, cell_first, ragged_right, ea);
        const int d = tb.d;
        using View = PhmSlice;
        View b0 = View::at(slice, W, 0), b1 = View::at(slice, W, 1), b2 = View::at(slice, W, 2);
        int l1 = 1, r1 = 0, l2 = 1, r2 = 0; /* the limits of d' + 1 and d' + 2: empty beyond d */
        PstCand *__restrict__ list_m = cand_m + tb.cand_base;
        PstCand *__restrict__ list_x = with_gaps ? cand_x + tb.cand_base : nullptr;
        PstCand *__restrict__ list_y = with_gaps ? cand_y + tb.cand_base : nullptr;
        int n_m = 0, n_x = 0, n_y = 0;
        int taken = 0; /* totalPosteriorCalculationsThisTraceback */
        double total = PHM_NEG;
        for (int dd = d; dd > tb.to; dd--) {
            const int l0 = s.bnd[2 * dd], r0 = s.bnd[2 * dd + 1];
            const int width = (r0 - l0) / 2 + 1;
            if (dd == d) {
                for (int i = tid; i < width; i += T) b0.store(i, St{s.e_end[0], s.e_end[1], s.e_end[2]});
            } else {
                for (int i = tid; i < width; i += T) b0.store(i, pst_backward_cell(dd, l0 + 2 * i, l1, r1, l2, r2, b1, b2, s.c));
            }
            __syncthreads();
            if (dd <= tb.from) {
                /* (the first cell folded into the pointers: 78 VGPRs against 82 at 128 threads, an occupancy step) */
                const PhmPlanarT<const double> fwd{ws_m + s.first[dd], ws_x + s.first[dd], ws_y + s.first[dd], 0};
                if (taken % 10 == 0) {
                    /* diagonalCalculationTotalProbability (:578-596): the cells' terms side by side */
                    for (int i = tid; i < width; i += T) term[i] = pst_total_term_here(fwd.load(i), b0.load(i));
                    const bool second = dd < d; /* diagonal dd + 1 has a backward diagonal; the forward diagonal dd - 1 always exists */
                    const int width1 = second ? (r1 - l1) / 2 + 1 : 0;
                    if (second) {
                        const int lm = s.bnd[2 * (dd - 1)], rm = s.bnd[2 * (dd - 1) + 1];
                        const PhmPlanarT<const double> fwd_m{ws_m, ws_x, ws_y, s.first[dd - 1]};
                        for (int j = tid; j < width1; j += T)
                            term[W + j] = pst_total_term_next(dd, l1 + 2 * j, lm, rm, fwd_m, b1.load(j), s.c);
                    }
                    __syncthreads();
                    /* dpDiagonal_dotProduct (:450-461) of either row: serially, ascending in x - y; phm_log_add is not associative, so no
                     * tree.  The two rows are two chains: the first wave folds one, the second wave the other */
                    if (wave == 0) {
                        const double a = pst_fold_row(term, width, lane);
                        if (lane == 0) row_total[0] = a;
                    } else if (wave == 1 && second) {
                        const double b = pst_fold_row(term + W, width1, lane);
                        if (lane == 0) row_total[1] = b;
                    }
                    __syncthreads();
                    total = second ? phm_log_add(row_total[0], row_total[1]) : row_total[0];
                    if (tid == 0 && dd == s.n) total_out[s.slot] = total;
                }
                taken++;
                /* diagonalCalculationPosteriorMatchProbs / ...PosteriorProbs (:610-681), ascending in x - y across the workgroup */
                for (int c0 = 0; c0 < width; c0 += T) {
                    const bool in = c0 + tid < width;
                    const int i = in ? c0 + tid : 0;
                    const int z = l0 + 2 * i;
                    const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                    double vm, vx = PHM_NEG, vy = PHM_NEG;
                    const bool keep_m = pst_candidate(0, in, x, y, fwd.load(i).m, b0.load(i).m, total, cut, vm);
                    const bool keep_x = with_gaps && pst_candidate(1, in, x, y, fwd.load(i).x, b0.load(i).x, total, cut, vx);
                    const bool keep_y = with_gaps && pst_candidate(2, in, x, y, fwd.load(i).y, b0.load(i).y, total, cut, vy);
                    const unsigned long long mask_m = __ballot(keep_m), mask_x = __ballot(keep_x), mask_y = __ballot(keep_y);
                    if (lane == 0) {
                        wave_count[flip][0][wave] = __popcll(mask_m);
                        wave_count[flip][1][wave] = __popcll(mask_x);
                        wave_count[flip][2][wave] = __popcll(mask_y);
                    }
                    __syncthreads();
                    int below[3] = {0, 0, 0}, all[3] = {0, 0, 0};
#pragma unroll
                    for (int w = 0; w < NW; w++)
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            const int cnt = wave_count[flip][q][w];
                            if (w < wave) below[q] += cnt;
                            all[q] += cnt;
                        }
                    const unsigned long long lower_lanes = (1ull << lane) - 1ull;
                    if (keep_m) list_m[n_m + below[0] + __popcll(mask_m & lower_lanes)] = PstCand{x - 1, y - 1, vm};
                    if (keep_x) list_x[n_x + below[1] + __popcll(mask_x & lower_lanes)] = PstCand{x - 1, y - 1, vx};
                    if (keep_y) list_y[n_y + below[2] + __popcll(mask_y & lower_lanes)] = PstCand{x - 1, y - 1, vy};
                    n_m += all[0];
                    n_x += all[1];
                    n_y += all[2];
                    flip ^= 1;
                }
            }
            /* (no barrier here: what the next diagonal writes -- b2 as its b0, the terms, the other half of the counts -- was last read
             * in front of a barrier every thread has passed before that write; the row totals are written behind the barrier that
             * follows the terms, which every reader of the previous ones has reached) */
            const View tmp = b2;
            b2 = b1; b1 = b0; b0 = tmp;
            l2 = l1; r2 = r1; l1 = l0; r1 = r0;
        }
        if (tid == 0) {
            counts[tb.slot] = n_m;
            counts[n_tb_group + tb.slot] = n_x;
            counts[2 * n_tb_group + tb.slot] = n_y;
        }
        __syncthreads(); /* the next traceback of this workgroup starts over in the slice a slower thread may still be reading */
    }
}
constexpr int PST_WIDE_THREADS = 1024;     /* workgroup of the two kernels (measured against 256 and 512: DESIGN.md 9.15) */
constexpr int PST_WIDE_HOOK_THREADS = 128; /* test hook bit 7: two waves, so that the suite's pairs cross waves and chunks */

/* dense[dense_first[list * n_tb + slot] + k] = the k-th candidate of traceback slot in list; a workgroup per (slot, list) */
__global__ void __launch_bounds__(256) pst_pack_kernel(const PstCand *__restrict__ cand, int64_t list_stride, const int64_t *__restrict__ cand_base,
                                                       const int32_t *__restrict__ counts, const int64_t *__restrict__ dense_first, int64_t n_tb,
                                                       PstCand *__restrict__ dense) {
    const int64_t slot = blockIdx.x, list = blockIdx.y;
    const int32_t n = counts[list * n_tb + slot];
    const PstCand *__restrict__ src = cand + list * list_stride + cand_base[slot];
    PstCand *__restrict__ dst = dense + dense_first[list * n_tb + slot];
    for (int32_t k = threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
}

struct PstList { /* one output list while the call builds it */
    std::vector<int64_t> first{0};
    std::vector<int32_t> x, y, weight;
    std::vector<double> v;
};

/* addPosteriorProb (:598-608) over the candidates of one traceback, in their order */
void pst_apply_rule(const PstCand *c, int64_t n, double threshold, PstList &out) {
    for (int64_t k = 0; k < n; k++) {
        double p = exp(c[k].v);
        if (!(p >= threshold)) continue;
        if (p > 1.0) p = 1.0;
        p = floor(p * 10000000.0); /* PAIR_ALIGNMENT_PROB_1 */
        out.x.push_back(c[k].x);
        out.y.push_back(c[k].y);
        out.weight.push_back((int32_t) (int64_t) p);
        out.v.push_back(c[k].v);
    }
}

int pst_hand_out(const PstList &L, mrp_posterior_pairs *out) {
    mrp_posterior_pairs r;
    r.first = (int64_t *) sc_dup(L.first.data(), L.first.size() * sizeof(int64_t));
    r.x = (int32_t *) sc_dup(L.x.data(), L.x.size() * sizeof(int32_t));
    r.y = (int32_t *) sc_dup(L.y.data(), L.y.size() * sizeof(int32_t));
    r.weight = (int32_t *) sc_dup(L.weight.data(), L.weight.size() * sizeof(int32_t));
    r.log_posterior = (double *) sc_dup(L.v.data(), L.v.size() * sizeof(double));
    if (!r.first || !r.x || !r.y || !r.weight || !r.log_posterior) {
        mrp_posterior_pairs_free(&r);
        return fail(MRP_ERR_NOMEM, "mrp_posterior_aligned_pairs: out of host memory");
    }
    *out = r;
    return MRP_OK;
}

/* What the host knows of a pair before anything is launched, and of the call: the bands and, from them alone, the tracebacks */
struct PstHostPair {
    int64_t band_first; /* its diagonal 0 in the call's band arrays */
    int64_t cells;
    int64_t tb_first;   /* its tracebacks in the call's plan */
    int32_t width;
};
struct PstPlan {
    std::vector<PstHostPair> pair;
    std::vector<int32_t> L, R;
    std::vector<PstTraceback> tbs;
    int64_t tb_end(int64_t i) const { return i + 1 < (int64_t) pair.size() ? pair[(size_t) i + 1].tb_first : (int64_t) tbs.size(); }
};

/* One group: its host arrays, reused from group to group.  Launch classes 0..3: the pair-per-wave kernels by LDS; class 4: the
 * pair-per-workgroup kernels.  Test hook bit 7 (wide_hook) sends every pair there, at PST_WIDE_HOOK_THREADS and a grid of one
 * workgroup, so that consecutive pairs and tracebacks reuse one slice. */
struct PstGroup {
    bool wide_hook;
    HostVec<PstPair> pairs[5];
    HostVec<PstTb> tbs[5];
    HostVec<int32_t> band, counts;
    HostVec<int64_t> cell_first, cand_base, dense_first;
    HostVec<PstCand> dense;
    HostVec<double> total;
    std::vector<int64_t> tb_slot0, pair_slot; /* per pair of the group: its first traceback slot, its own slot; -1: two empty strings */
    int wide_width;                           /* the widest diagonal of class 4 */
    int64_t wide_cells;                       /* its band cells */
    int64_t cell, cand, n_tb, n_slot;         /* band cells, candidate slots per list, tracebacks, pairs that are scored */
};

/* The device arrays of one group */
struct PstGroupDev {
    hipStream_t s = nullptr;
    DevBufGroup arrays;
    DevBuf<PstPair> d_pairs{arrays};
    DevBuf<PstTb> d_tbs{arrays};
    DevBuf<int32_t> d_band{arrays};
    DevBuf<int64_t> d_cell_first{arrays};
    DevBuf<double> d_ws{arrays};
    DevBuf<double> d_ws_back{arrays}; /* [workgroup of pst_traceback_wide_kernel][11 * widest diagonal] */
    DevBuf<PstCand> d_cand{arrays};
    DevBuf<int64_t> d_cand_base{arrays};
    DevBuf<int32_t> d_counts{arrays};
    DevBuf<int64_t> d_dense_first{arrays};
    DevBuf<PstCand> d_dense{arrays};
    DevBuf<double> d_total{arrays};
    ~PstGroupDev() {
        if (s) (void) hipStreamSynchronize(s);
    }
};

/* ---- MRP_ERR_ARG ---- */
int pst_check_arguments(const char *who, bool dynamic, const mrp_pair_hmm *models, int32_t n_models, const PhmPairs &P, const uint8_t *pool,
                        int64_t pool_bytes, const int64_t *anchor_expansion, const mrp_posterior_options *opt, const mrp_posterior_pairs *match_out,
                        const mrp_posterior_pairs *gap_x_out, const mrp_posterior_pairs *gap_y_out) {
    if (!models || !opt || !match_out || n_models <= 0 || P.n < 0 || pool_bytes < 0 || (pool_bytes > 0 && !pool))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (P.n > 0 && (!P.x_off || !P.x_len || !P.y_off || !P.y_len)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (P.n >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    if (const char *msg = pst_options_error(opt)) return mrp_set_error(MRP_ERR_ARG, "%s: %s", who, msg);
    if (opt->with_gaps != 0 && opt->with_gaps != 1) return mrp_set_error(MRP_ERR_ARG, "%s: with_gaps must be 0 or 1", who);
    if ((opt->with_gaps != 0) != (gap_x_out != nullptr) || (opt->with_gaps != 0) != (gap_y_out != nullptr))
        return mrp_set_error(MRP_ERR_ARG, "%s: gap_x_out and gap_y_out must be given exactly when with_gaps is set", who);
    for (int64_t i = 0; i < P.n; i++) {
        const int64_t lx = P.x_len[i], ly = P.y_len[i];
        const int64_t na = P.anchor_off ? P.anchor_off[i + 1] - P.anchor_off[i] : 0;
        if (lx < 0 || ly < 0 || P.x_off[i] < 0 || P.y_off[i] < 0 || P.x_off[i] + lx > pool_bytes || P.y_off[i] + ly > pool_bytes ||
            (P.anchor_off && P.anchor_off[i] < 0) || na < 0 || (na > 0 && (!P.anchors || (dynamic && !anchor_expansion))))
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld lies outside the symbol pool or has bad anchor offsets", who, (long long) i);
        if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld: strings too long", who, (long long) i);
    }
    for (int64_t i = 0; i < P.n; i++)
        if (P.model && P.model[i] >= n_models)
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld names model %d of %d", who, (long long) i, (int) P.model[i], (int) n_models);
    return MRP_OK;
}

/* the bands (band_construct, :175-226, or band_constructDynamic, :120-173) and, from them alone, the tracebacks; still MRP_ERR_ARG */
int pst_bands_and_plan(const char *who, bool dynamic, const PhmPairs &P, const int64_t *anchor_expansion, const mrp_posterior_options *opt, PstPlan &plan,
                       int64_t &cells_all) {
    plan.pair.resize((size_t) P.n);
    int64_t n_diags = 0;
    for (int64_t i = 0; i < P.n; i++) {
        const int64_t lx = P.x_len[i], ly = P.y_len[i], n = lx + ly;
        const int64_t na = P.anchor_off ? P.anchor_off[i + 1] - P.anchor_off[i] : 0;
        plan.L.resize((size_t) (n_diags + n + 1));
        plan.R.resize((size_t) (n_diags + n + 1));
        PstHostPair &h = plan.pair[(size_t) i];
        h.band_first = n_diags;
        int width = 1;
        if (band_closed_form_any(na > 0 ? P.anchors + 2 * P.anchor_off[i] : nullptr, dynamic && na > 0 ? anchor_expansion + P.anchor_off[i] : nullptr, dynamic, na, lx,
                                 ly, opt->expansion, plan.L.data() + n_diags, plan.R.data() + n_diags, &h.cells, &width) != MRP_OK)
            return mrp_set_error(MRP_ERR_ARG, dynamic ? "%s: pair %lld has invalid anchors or an odd or negative anchor expansion (pairwiseAligner.c:151-158)"
                                                      : "%s: pair %lld has invalid anchors (pairwiseAligner.c:206-211)",
                                 who, (long long) i);
        h.width = width;
        h.tb_first = (int64_t) plan.tbs.size();
        pst_plan_tracebacks(plan.L.data() + n_diags, plan.R.data() + n_diags, n, opt->expansion, opt->min_diags_between_traceback, opt->traceback_diagonals, plan.tbs);
        n_diags += n + 1;
        cells_all += h.cells;
    }
    return MRP_OK;
}

/* ---- MRP_ERR_UNSUPPORTED ---- */
int pst_check_supported(const char *who, bool wide_on, int64_t budget, const PstPlan &plan) {
    const int64_t n_pairs = (int64_t) plan.pair.size();
    for (int64_t i = 0; i < n_pairs; i++) {
        const int width = (int) plan.pair[(size_t) i].width;
        if (width <= PHM_WAVE_MAX_WIDTH) continue;
        if (!wide_on)
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d; wide pairs are not extended to this entry)", who,
                                 (long long) i, width, PHM_WAVE_MAX_WIDTH);
        if (width > MRP_WIDE_MAX_WIDTH)
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d with posterior wide pairs on, MRP_WIDE_MAX_WIDTH)", who,
                                 (long long) i, width, (int) MRP_WIDE_MAX_WIDTH);
    }
    for (int64_t i = 0; i < n_pairs; i++)
        if (plan.pair[(size_t) i].cells * PST_CELL_BYTES > budget)
            return mrp_set_error(MRP_ERR_UNSUPPORTED,
                                 "%s: pair %lld keeps %lld band cells, %lld bytes of forward diagonals (limit %lld bytes, mrp_context_set_posterior_workspace)", who,
                                 (long long) i, (long long) plan.pair[(size_t) i].cells, (long long) (plan.pair[(size_t) i].cells * PST_CELL_BYTES), (long long) budget);
    for (int64_t i = 0; i < n_pairs; i++) /* (a traceback counts its candidates in 32 bits) */
        if (plan.pair[(size_t) i].cells >= (1ll << 31))
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld keeps %lld band cells (limit 2^31 - 1 whatever the workspace)", who, (long long) i,
                                 (long long) plan.pair[(size_t) i].cells);
    return MRP_OK;
}

/* The host half of the group of pairs [g0, g1): the pairs classed, PstPair / PstTb, the bands and the candidate bases */
void pst_group_build(const PhmPairs &P, const PstPlan &plan, int64_t g0, int64_t g1, bool wide_hook, PstGroup &G, mrp_posterior_stats &ps) {
    G.wide_hook = wide_hook;
    for (int c = 0; c < 5; c++) { G.pairs[c].clear(); G.tbs[c].clear(); }
    G.wide_width = 1;
    G.wide_cells = 0;
    G.band.clear();
    G.cell_first.clear();
    G.cand_base.clear();
    G.cell = G.cand = G.n_tb = G.n_slot = 0;
    G.tb_slot0.assign((size_t) (g1 - g0), -1);
    G.pair_slot.assign((size_t) (g1 - g0), -1);
    for (int64_t i = g0; i < g1; i++) {
        const PstHostPair &h = plan.pair[(size_t) i];
        const int64_t n = (int64_t) P.x_len[i] + P.y_len[i];
        if (n == 0) continue; /* two empty strings: no lists, a total of 0.0 (:721-723) */
        int c = 0;
        if (wide_hook || h.width > PHM_WAVE_MAX_WIDTH) {
            c = 4;
            G.wide_width = std::max(G.wide_width, (int) h.width);
            G.wide_cells += h.cells;
        } else {
            while (h.width > WAVE_CLASS_CAP[c]) c++;
        }
        const PstPair p{P.x_off[i], P.y_off[i], (int64_t) G.cell_first.size(), P.x_len[i], P.y_len[i], P.model ? P.model[i] : 0, (int32_t) G.n_slot};
        G.pair_slot[(size_t) (i - g0)] = G.n_slot++;
        for (int64_t d = 0; d <= n; d++) {
            const int32_t l = plan.L[(size_t) (h.band_first + d)], r = plan.R[(size_t) (h.band_first + d)];
            G.band.push_back(l);
            G.band.push_back(r);
            G.cell_first.push_back(G.cell);
            G.cell += (r - l) / 2 + 1;
        }
        /* the band cells of the pair's diagonals (to, from] */
        const auto cells_between = [&](int64_t to, int64_t from) {
            return G.cell_first[(size_t) (p.diag0 + from)] + (plan.R[(size_t) (h.band_first + from)] - plan.L[(size_t) (h.band_first + from)]) / 2 + 1 -
                   G.cell_first[(size_t) (p.diag0 + to + 1)];
        };
        G.tb_slot0[(size_t) (i - g0)] = G.n_tb;
        for (int64_t k = h.tb_first; k < plan.tb_end(i); k++) {
            const PstTraceback &q = plan.tbs[(size_t) k];
            G.tbs[c].push_back(PstTb{(int32_t) G.pairs[c].size(), (int32_t) q.d, (int32_t) q.to, (int32_t) q.from, G.n_tb++, G.cand});
            G.cand_base.push_back(G.cand);
            G.cand += cells_between(q.to, q.from); /* at most one candidate per list and cell */
            ps.traceback_cells += cells_between(q.to, q.d);
        }
        G.pairs[c].push_back(p);
    }
}

/* launch(std::integral_constant<int, T>): the workgroup of the pair-per-workgroup kernels, the test hook's or the full one */
template <class F>
void pst_with_wide_threads(bool wide_hook, F launch) {
    if (wide_hook) launch(std::integral_constant<int, PST_WIDE_HOOK_THREADS>{});
    else launch(std::integral_constant<int, PST_WIDE_THREADS>{});
}

/* launch(PstEmission<Em>{}, args): the match emission of the call, the nucleotide one or (rle) the run-length one */
template <class Em>
struct PstEmission {
    using type = Em;
};
template <class F>
void pst_with_emission(const PhmRunLength::Args *rle, F launch) {
    if (rle) launch(PstEmission<PhmRunLength>{}, *rle);
    else launch(PstEmission<PhmNucleotide>{}, PhmNucleotide::Args{});
}

/* The device half of a group with at least one scored pair: uploads, the forward and traceback launches between the context's events,
 * the counts, the pack and the download of the dense candidates into H.dense */
int pst_group_run(mrp_context *ctx, const uint8_t *d_pool, const PhmModelDev *d_models, const PhmRunLength::Args *rle, const mrp_posterior_options *opt, PstGroup &H,
                  mrp_posterior_stats &ps) {
    hipStream_t s = ctx->stream;
    const int n_lists = opt->with_gaps ? 3 : 1;
    const int with_gaps = (int) opt->with_gaps, ragged_right = (int) (opt->ragged_right != 0);
    const double cut = log(opt->threshold) - 1e-6; /* wider than the rule by far more than exp() errs: the host decides */
    const int64_t cell = H.cell, cand = H.cand, n_tb = H.n_tb, n_slot = H.n_slot;
    PstGroupDev G;
    G.arrays.bind(&ctx->pool);
    G.s = s;
    /* one array of pairs and one of tracebacks, class after class */
    HostVec<PstPair> all_pairs;
    HostVec<PstTb> all_tbs;
    int64_t pair0[6] = {0, 0, 0, 0, 0, 0}, tb0[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 5; c++) {
        all_pairs.insert(all_pairs.end(), H.pairs[c].begin(), H.pairs[c].end());
        all_tbs.insert(all_tbs.end(), H.tbs[c].begin(), H.tbs[c].end());
        pair0[c + 1] = (int64_t) all_pairs.size();
        tb0[c + 1] = (int64_t) all_tbs.size();
    }
    PHM_HIP(G.d_pairs.upload(all_pairs, s));
    PHM_HIP(G.d_tbs.upload(all_tbs, s));
    PHM_HIP(G.d_band.upload(H.band, s));
    PHM_HIP(G.d_cell_first.upload(H.cell_first, s));
    PHM_HIP(G.d_cand_base.upload(H.cand_base, s));
    PHM_HIP(G.d_ws.alloc(3 * (size_t) cell));
    PHM_HIP(G.d_cand.alloc((size_t) n_lists * (size_t) cand));
    PHM_HIP(G.d_counts.alloc(3 * (size_t) n_tb));
    PHM_HIP(G.d_total.alloc((size_t) n_slot));
    double *ws_m = G.d_ws.p, *ws_x = G.d_ws.p + cell, *ws_y = G.d_ws.p + 2 * cell;
    /* class 4: a slice of backward diagonals per workgroup of the traceback kernel, as many as PHM_WIDE_WORKSPACE_BYTES holds */
    const int64_t n_wide = pair0[5] - pair0[4], n_wide_tb = tb0[5] - tb0[4];
    const int64_t slice_doubles = 11 * (int64_t) H.wide_width;
    const int64_t wide_fgrid = H.wide_hook ? 1 : std::min<int64_t>(n_wide, 1 << 20);
    const int64_t wide_tgrid =
        H.wide_hook ? 1 : std::min<int64_t>(n_wide_tb, std::max<int64_t>(1, PHM_WIDE_WORKSPACE_BYTES / (slice_doubles * (int64_t) sizeof(double))));
    if (n_wide_tb > 0) PHM_HIP(G.d_ws_back.alloc((size_t) (wide_tgrid * slice_doubles)));
    PHM_HIP(hipStreamSynchronize(s)); /* the uploads are not part of the kernels' time */
    PHM_HIP(hipEventRecord(ctx->ev[0], s));
    for (int c = 0; c < 4; c++) {
        const int64_t n = pair0[c + 1] - pair0[c];
        if (n == 0) continue;
        const int W = WAVE_CLASS_CAP[c];
        pst_with_emission(rle, [&](auto em, auto ea) {
            using Em = typename decltype(em)::type;
            hipLaunchKernelGGL(pst_forward_kernel<Em>, dim3((unsigned) std::min<int64_t>(n, 1 << 20)), dim3(PHM_WAVE), (size_t) 9 * W * sizeof(double), s,
                               G.d_pairs.p + pair0[c], n, d_pool, d_models, G.d_band.p, G.d_cell_first.p, W, ws_m, ws_x, ws_y, ea);
        });
        PHM_HIP(hipGetLastError());
    }
    if (n_wide > 0) {
        pst_with_wide_threads(H.wide_hook, [&](auto threads) {
            constexpr int T = decltype(threads)::value;
            pst_with_emission(rle, [&](auto em, auto ea) {
                using Em = typename decltype(em)::type;
                hipLaunchKernelGGL((pst_forward_wide_kernel<T, Em>), dim3((unsigned) wide_fgrid), dim3(T), 0, s, G.d_pairs.p + pair0[4], n_wide, d_pool, d_models,
                                   G.d_band.p, G.d_cell_first.p, ws_m, ws_x, ws_y, ea);
            });
        });
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ctx->ev[1], s));
    for (int c = 0; c < 4; c++) {
        const int64_t n = tb0[c + 1] - tb0[c];
        if (n == 0) continue;
        const int W = WAVE_CLASS_CAP[c];
        pst_with_emission(rle, [&](auto em, auto ea) {
            using Em = typename decltype(em)::type;
            hipLaunchKernelGGL(pst_traceback_kernel<Em>, dim3((unsigned) n), dim3(PHM_WAVE), (size_t) 9 * W * sizeof(double), s, G.d_pairs.p + pair0[c],
                               G.d_tbs.p + tb0[c], d_pool, d_models, G.d_band.p, G.d_cell_first.p, W, ws_m, ws_x, ws_y, cut, with_gaps, ragged_right, n_tb, G.d_cand.p,
                               G.d_cand.p + cand, G.d_cand.p + 2 * cand, G.d_counts.p, G.d_total.p, ea);
        });
        PHM_HIP(hipGetLastError());
    }
    if (n_wide_tb > 0) {
        pst_with_wide_threads(H.wide_hook, [&](auto threads) {
            constexpr int T = decltype(threads)::value;
            pst_with_emission(rle, [&](auto em, auto ea) {
                using Em = typename decltype(em)::type;
                hipLaunchKernelGGL((pst_traceback_wide_kernel<T, Em>), dim3((unsigned) wide_tgrid), dim3(T), 0, s, G.d_pairs.p + pair0[4], G.d_tbs.p + tb0[4],
                                   n_wide_tb, d_pool, d_models, G.d_band.p, G.d_cell_first.p, H.wide_width, ws_m, ws_x, ws_y, G.d_ws_back.p, cut, with_gaps,
                                   ragged_right, n_tb, G.d_cand.p, G.d_cand.p + cand, G.d_cand.p + 2 * cand, G.d_counts.p, G.d_total.p, ea);
            });
        });
        PHM_HIP(hipGetLastError());
    }
    ctx->posterior_wide_count += n_wide;
    ctx->posterior_wide_cells += H.wide_cells;
    PHM_HIP(hipEventRecord(ctx->ev[2], s));
    H.counts.resize(3 * (size_t) n_tb);
    H.total.resize((size_t) n_slot);
    PHM_HIP(hipMemcpyAsync(H.counts.data(), G.d_counts.p, 3 * (size_t) n_tb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PHM_HIP(hipMemcpyAsync(H.total.data(), G.d_total.p, (size_t) n_slot * sizeof(double), hipMemcpyDeviceToHost, s));
    PHM_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ps.forward_ms += ms;
    PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
    ps.traceback_ms += ms;
    H.dense_first.resize((size_t) n_lists * (size_t) n_tb);
    int64_t n_dense = 0;
    for (int l = 0; l < n_lists; l++)
        for (int64_t k = 0; k < n_tb; k++) {
            H.dense_first[(size_t) (l * n_tb + k)] = n_dense;
            n_dense += H.counts[(size_t) (l * n_tb + k)];
        }
    H.dense.resize((size_t) n_dense);
    if (n_dense > 0) {
        PHM_HIP(G.d_dense_first.upload(H.dense_first, s));
        PHM_HIP(G.d_dense.alloc((size_t) n_dense));
        hipLaunchKernelGGL(pst_pack_kernel, dim3((unsigned) n_tb, (unsigned) n_lists), dim3(256), 0, s, G.d_cand.p, cand, G.d_cand_base.p, G.d_counts.p,
                           G.d_dense_first.p, n_tb, G.d_dense.p);
        PHM_HIP(hipGetLastError());
        PHM_HIP(hipMemcpyAsync(H.dense.data(), G.d_dense.p, (size_t) n_dense * sizeof(PstCand), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipStreamSynchronize(s));
    }
    ps.candidates += n_dense;
    ps.downloaded_bytes += n_dense * (int64_t) sizeof(PstCand) + 3 * n_tb * (int64_t) sizeof(int32_t) + n_slot * (int64_t) sizeof(double);
    return MRP_OK;
}

/* The host's rule over the group's candidates, pair by pair in input order, traceback by traceback */
void pst_group_rule(const PstPlan &plan, int64_t g0, int64_t g1, const PstGroup &G, int n_lists, double threshold, PstList *lists, std::vector<double> &totals) {
    for (int64_t i = g0; i < g1; i++) {
        const int64_t slot = G.pair_slot[(size_t) (i - g0)];
        if (slot >= 0) {
            totals[(size_t) i] = G.total[(size_t) slot];
            const int64_t k0 = G.tb_slot0[(size_t) (i - g0)], k1 = k0 + (plan.tb_end(i) - plan.pair[(size_t) i].tb_first);
            for (int l = 0; l < n_lists; l++)
                for (int64_t k = k0; k < k1; k++)
                    pst_apply_rule(G.dense.data() + G.dense_first[(size_t) (l * G.n_tb + k)], G.counts[(size_t) (l * G.n_tb + k)], threshold, lists[l]);
        }
        for (int l = 0; l < n_lists; l++) lists[l].first.push_back((int64_t) lists[l].x.size());
    }
}

}  // namespace

extern "C" {

void mrp_posterior_pairs_free(mrp_posterior_pairs *p) {
    if (!p) return;
    free(p->first);
    free(p->x);
    free(p->y);
    free(p->weight);
    free(p->log_posterior);
    memset(p, 0, sizeof(*p));
}

int mrp_posterior_tracebacks(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, const mrp_posterior_options *opt,
                             int64_t *triples_out, int64_t capacity, int64_t *n_out) {
    static const char *who = "mrp_posterior_tracebacks";
    if (!opt || !n_out || (n_anchors > 0 && !anchors) || n_anchors < 0 || capacity < 0 || (capacity > 0 && !triples_out))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or negative count", who);
    if (const char *msg = pst_options_error(opt)) return mrp_set_error(MRP_ERR_ARG, "%s: %s", who, msg);
    if (lx < 0 || ly < 0 || lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: bad string lengths", who);
    const int64_t n = lx + ly;
    std::vector<int32_t> L((size_t) n + 1), R((size_t) n + 1);
    if (band_closed_form(anchors, n_anchors, lx, ly, opt->expansion, L.data(), R.data(), nullptr, nullptr) != MRP_OK)
        return mrp_set_error(MRP_ERR_ARG, "%s: invalid anchors (pairwiseAligner.c:206-211)", who);
    std::vector<PstTraceback> plan;
    pst_plan_tracebacks(L.data(), R.data(), n, opt->expansion, opt->min_diags_between_traceback, opt->traceback_diagonals, plan);
    *n_out = (int64_t) plan.size();
    for (int64_t k = 0; k < std::min<int64_t>(capacity, (int64_t) plan.size()); k++) {
        triples_out[3 * k] = plan[(size_t) k].d;
        triples_out[3 * k + 1] = plan[(size_t) k].to;
        triples_out[3 * k + 2] = plan[(size_t) k].from;
    }
    return MRP_OK;
}

int mrp_context_set_posterior_workspace(mrp_context *ctx, int64_t bytes) {
    if (!ctx) return mrp_set_error(MRP_ERR_ARG, "mrp_context_set_posterior_workspace: context is NULL");
    if (bytes < 0) return mrp_set_error(MRP_ERR_ARG, "mrp_context_set_posterior_workspace: negative size");
    ctx->posterior_workspace = bytes; /* 0: the default */
    return MRP_OK;
}

int mrp_context_last_posterior(mrp_context *ctx, mrp_posterior_stats *out) {
    if (!ctx || !out) return mrp_set_error(MRP_ERR_ARG, "mrp_context_last_posterior: null argument");
    *out = ctx->last_posterior;
    return MRP_OK;
}

int mrp_context_set_posterior_wide_pairs(mrp_context *ctx, int on) {
    if (!ctx) return mrp_set_error(MRP_ERR_ARG, "mrp_context_set_posterior_wide_pairs: context is NULL");
    ctx->posterior_wide_pairs = on != 0;
    return MRP_OK;
}

int mrp_context_posterior_wide_count(mrp_context *ctx, int64_t *pairs_out, int64_t *cells_out) {
    if (!ctx) return mrp_set_error(MRP_ERR_ARG, "mrp_context_posterior_wide_count: context is NULL");
    if (pairs_out) *pairs_out = ctx->posterior_wide_count;
    if (cells_out) *cells_out = ctx->posterior_wide_cells;
    return MRP_OK;
}

/* The entries.  repeat: run-length emissions (the two arguments of the _rle entry), else the nucleotide ones.  dynamic: the band is band_constructDynamic's over anchor_expansion (one per anchor, indexed as the anchors are);
 * else band_construct's over opt->expansion.  Everything behind the band is the same call.  The order of the error classes is part of
 * the contract: MRP_ERR_ARG, then MRP_ERR_UNSUPPORTED, then MRP_ERR_NO_DEVICE. */
static int pst_aligned_pairs(const char *who, bool dynamic, mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, const PhmPairs &P,
                             const uint8_t *pool, int64_t pool_bytes, const int64_t *anchor_expansion, const mrp_posterior_options *opt,
                             mrp_posterior_pairs *match_out, mrp_posterior_pairs *gap_x_out, mrp_posterior_pairs *gap_y_out, double *total_out,
                             mrp_pairhmm_stats *stats, bool run_length = false, const mrp_repeat_model *repeat = nullptr, const uint8_t *counts = nullptr) {
    const double t_begin = now_ms();
    const int64_t n_pairs = P.n;
    int rc = pst_check_arguments(who, dynamic, models, n_models, P, pool, pool_bytes, anchor_expansion, opt, match_out, gap_x_out, gap_y_out);
    if (rc != MRP_OK) return rc;
    PhmRle rle;
    if (run_length) {
        rc = phm_rle_check_and_build(who, repeat, n_models, counts, P, rle);
        if (rc != MRP_OK) return rc;
    }
    PstPlan plan;
    mrp_posterior_stats ps;
    memset(&ps, 0, sizeof(ps));
    rc = pst_bands_and_plan(who, dynamic, P, anchor_expansion, opt, plan, ps.cells);
    if (rc != MRP_OK) return rc;
    const int64_t budget = ctx && ctx->posterior_workspace > 0 ? ctx->posterior_workspace : PST_DEFAULT_WORKSPACE;
    rc = pst_check_supported(who, ctx && ctx->posterior_wide_pairs, budget, plan);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the pair-HMM path has no CPU fallback)", who);

    const int n_lists = opt->with_gaps ? 3 : 1;
    PstList lists[3];
    std::vector<double> totals((size_t) n_pairs, 0.0);
    std::vector<PhmModelDev> hm((size_t) n_models);
    for (int i = 0; i < n_models; i++) model_to_device(models[i], opt->ragged_left != 0, opt->ragged_right != 0, hm[(size_t) i]);
    int64_t n_scored = 0;
    if (n_pairs > 0) {
        PHM_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        static PerDeviceOnce once;
        const hipError_t configured = once.run([] {
            constexpr int lds = 9 * PHM_WAVE_MAX_WIDTH * (int) sizeof(double);
            const void *kernels[4] = {(const void *) pst_forward_kernel<PhmNucleotide>, (const void *) pst_traceback_kernel<PhmNucleotide>,
                                      (const void *) pst_forward_kernel<PhmRunLength>, (const void *) pst_traceback_kernel<PhmRunLength>};
            hipError_t e = hipSuccess;
            for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            return e;
        });
        PHM_HIP(configured);
        DevBuf<PhmModelDev> d_models;
        DevBuf<uint8_t> d_pool;
        d_models.pool = d_pool.pool = &ctx->pool;
        PhmRleDev d_rle; /* the counts and tables of a run-length call */
        Drain drain{s};
        PHM_HIP(d_models.upload(hm, s));
        PHM_HIP(d_pool.alloc((size_t) pool_bytes));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));
        if (run_length) PHM_HIP(d_rle.upload(&ctx->pool, rle, pool_bytes, s));
        const PhmRunLength::Args rle_args{d_rle.d_counts.p, d_rle.d_models.p};

        /* the groups: consecutive pairs whose forward diagonals fit the workspace together */
        PstGroup G;
        for (int64_t g0 = 0; g0 < n_pairs;) {
            int64_t g1 = g0, g_cells = 0;
            while (g1 < n_pairs && (g1 == g0 || (g_cells + plan.pair[(size_t) g1].cells) * PST_CELL_BYTES <= budget)) g_cells += plan.pair[(size_t) g1++].cells;
            pst_group_build(P, plan, g0, g1, (ctx->test_hooks & 128) != 0, G, ps);
            ps.groups++;
            n_scored += G.n_slot;
            if (G.n_slot > 0) {
                rc = pst_group_run(ctx, d_pool.p, d_models.p, run_length ? &rle_args : nullptr, opt, G, ps);
                if (rc != MRP_OK) return rc;
            }
            ctx->pool.reclaim(); /* the group's arrays are idle: the next group takes them */
            pst_group_rule(plan, g0, g1, G, n_lists, opt->threshold, lists, totals);
            g0 = g1;
        }
    }
    ctx->pool.reclaim();
    /* nothing has been written so far: hand out */
    mrp_posterior_pairs r[3];
    memset(r, 0, sizeof(r));
    for (int l = 0; l < n_lists; l++) {
        rc = pst_hand_out(lists[l], &r[l]);
        if (rc != MRP_OK) {
            for (int q = 0; q < l; q++) mrp_posterior_pairs_free(&r[q]);
            return rc;
        }
    }
    *match_out = r[0];
    if (opt->with_gaps) {
        *gap_x_out = r[1];
        *gap_y_out = r[2];
    }
    if (total_out)
        for (int64_t i = 0; i < n_pairs; i++) total_out[i] = totals[(size_t) i];
    ps.total_ms = now_ms() - t_begin;
    ctx->last_posterior = ps;
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->pairs_wave = n_scored;
        stats->cells = ps.cells;
        stats->kernel_ms = ps.forward_ms + ps.traceback_ms;
        stats->total_ms = ps.total_ms;
    }
    return MRP_OK;
}

int mrp_posterior_aligned_pairs(mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, int64_t n_pairs, const uint8_t *pool,
                                int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len, const int64_t *y_off, const int32_t *y_len,
                                const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors, const mrp_posterior_options *opt,
                                mrp_posterior_pairs *match_out, mrp_posterior_pairs *gap_x_out, mrp_posterior_pairs *gap_y_out,
                                double *total_out, mrp_pairhmm_stats *stats) {
    return pst_aligned_pairs("mrp_posterior_aligned_pairs", false, ctx, models, n_models, PhmPairs{n_pairs, x_off, x_len, y_off, y_len, model_index, anchor_off, anchors},
                             pool, pool_bytes, nullptr, opt, match_out, gap_x_out, gap_y_out, total_out, stats);
}

int mrp_posterior_aligned_pairs_dynamic(mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, int64_t n_pairs, const uint8_t *pool,
                                        int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len, const int64_t *y_off, const int32_t *y_len,
                                        const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors, const int64_t *anchor_expansion,
                                        const mrp_posterior_options *opt, mrp_posterior_pairs *match_out, mrp_posterior_pairs *gap_x_out,
                                        mrp_posterior_pairs *gap_y_out, double *total_out, mrp_pairhmm_stats *stats) {
    return pst_aligned_pairs("mrp_posterior_aligned_pairs_dynamic", true, ctx, models, n_models,
                             PhmPairs{n_pairs, x_off, x_len, y_off, y_len, model_index, anchor_off, anchors}, pool, pool_bytes, anchor_expansion, opt, match_out,
                             gap_x_out, gap_y_out, total_out, stats);
}

int mrp_posterior_aligned_pairs_rle(mrp_context *ctx, const mrp_pair_hmm *models, const mrp_repeat_model *repeat, int32_t n_models, int64_t n_pairs,
                                    const uint8_t *pool, const uint8_t *counts, int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len,
                                    const int64_t *y_off, const int32_t *y_len, const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors,
                                    const int64_t *anchor_expansion, const mrp_posterior_options *opt, mrp_posterior_pairs *match_out,
                                    mrp_posterior_pairs *gap_x_out, mrp_posterior_pairs *gap_y_out, double *total_out, mrp_pairhmm_stats *stats) {
    return pst_aligned_pairs("mrp_posterior_aligned_pairs_rle", anchor_expansion != nullptr, ctx, models, n_models,
                             PhmPairs{n_pairs, x_off, x_len, y_off, y_len, model_index, anchor_off, anchors}, pool, pool_bytes, anchor_expansion, opt, match_out,
                             gap_x_out, gap_y_out, total_out, stats, true, repeat, counts);
}

}  // extern "C"
