/*
 * mrp_posterior.hip -- the posterior half of the banded pairwise aligner: getPosteriorProbsWithBanding
 * (impl/pairwiseAligner.c:706-844) with diagonalCalculationPosteriorMatchProbs (:610-635) or diagonalCalculationPosteriorProbs
 * (:637-681) for batches of string pairs.  gfx950 only; compiled with -ffp-contract=off.  DESIGN.md 9.15.
 *
 * The reference walks a pair's band forward and, at the diagonals the band alone decides (mrp_posterior_plan.h), walks a stretch of it
 * back.  Once the forward diagonals exist the tracebacks do not depend on one another, so the device runs them side by side:
 *
 *   pst_forward_kernel     a pair per wave, the walk of phm_wave_kernel (the same limits, phm_cell, phm_log_add), which also stores
 *                          every band cell's three states into the pair's slice of a workspace, an array per state.
 *   pst_traceback_kernel   a (pair, traceback) per wave: three backward diagonals rotate in LDS, the forward ones are read from the
 *                          workspace.  The reference pushes from a cell into its three predecessors (cell_calculateBackward, :322-331);
 *                          a lane here gathers a cell from its three successors in the order the pushes arrive (below).  The totals
 *                          (:578-596) are folded by one lane in index order.  Cells whose log posterior reaches a cut the host put a
 *                          little below log(threshold) are compacted, by ballot, into space sized from the plan.
 *   pst_pack_kernel        moves the candidates of the tracebacks behind one another: what is downloaded is 16 B per candidate.
 *   pst_forward_wide_kernel, pst_traceback_wide_kernel
 *                          the same two walks with a workgroup per pair / per (pair, traceback), for the pairs whose widest diagonal
 *                          exceeds the 2 048 cells the LDS of the two above holds (mrp_context_set_posterior_wide_pairs).
 *
 * The band is the host's, (l, r) per diagonal: band_construct's for mrp_posterior_aligned_pairs, band_constructDynamic's for
 * mrp_posterior_aligned_pairs_dynamic (mrp_band.h); the kernels do not know which.
 *
 * In the pair-per-wave kernels a workgroup is one wave and what it hands from step to step lives in LDS, so the barrier between steps is
 * lds_barrier(), which orders LDS traffic only: nothing in them reads what it stored to the workspace or to the lists.
 *
 * The host applies the reference's rule (addPosteriorProb, :598-608) with the C library's exp and keeps the order of generation.
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
#include "mrp_pairhmm_dev.h"
#include "mrp_posterior_plan.h"
#include "mrp_wave.h" /* lds_barrier */

#pragma clang fp contract(off)

namespace {

constexpr int64_t PST_DEFAULT_WORKSPACE = (int64_t) MRP_POSTERIOR_DEFAULT_WORKSPACE;
constexpr int64_t PST_CELL_BYTES = 24; /* three states of a band cell */

struct PstPair {
    int64_t x_off, y_off;
    int64_t diag0; /* the pair's diagonal 0 in band (pairs of int32) and in cell_first */
    int32_t lx, ly, model, slot; /* slot: the pair within its group, where its total goes */
};
struct PstTb {
    int32_t pair; /* within the launch class */
    int32_t d, to, from;
    int64_t slot;      /* the traceback within its group: where its counts go */
    int64_t cand_base; /* its first candidate slot, the same in every list */
};
struct PstCand {
    int32_t x, y; /* sequence coordinates, -1 for the gap before the first symbol */
    double v;     /* the log posterior whose exp() the host tests */
};
static_assert(sizeof(PstCand) == 16, "a candidate is 16 bytes");

static __device__ __forceinline__ int pst_sym(const uint8_t *__restrict__ s, int i) {
    const int c = s[i];
    return c > 4 ? 4 : c;
}

/* phm_wave_kernel with its diagonals kept: ws_m / ws_x / ws_y [cell_first[diag0 + d] + i] = cell i of diagonal d */
__global__ void __launch_bounds__(PHM_WAVE) pst_forward_kernel(const PstPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                                 const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band,
                                                                 const int64_t *__restrict__ cell_first, int W, double *__restrict__ ws_m,
                                                                 double *__restrict__ ws_x, double *__restrict__ ws_y) {
    extern __shared__ double pst_lds[]; /* 3 diagonals x W cells x 3 states */
    const int lane = threadIdx.x;
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PstPair p = pairs[pi];
        const int lx = p.lx, ly = p.ly, n = lx + ly;
        const PhmModelDev *__restrict__ M = models + p.model;
        double t[9];
#pragma unroll
        for (int i = 0; i < 9; i++) t[i] = M->t[i];
        const uint8_t *__restrict__ sx = pool + p.x_off;
        const uint8_t *__restrict__ sy = pool + p.y_off;
        double *d0 = pst_lds, *d1 = pst_lds + 3 * W, *d2 = pst_lds + 6 * W; /* being written, xay - 1, xay - 2 */
        auto limits = [&](int d, int &l, int &r) {
            l = band[2 * (p.diag0 + d)];
            r = band[2 * (p.diag0 + d) + 1];
        };
        int l1, r1, l2 = 1, r2 = 0;
        limits(0, l1, r1);
        {
            const int64_t base = cell_first[p.diag0];
            for (int i = lane; i <= (r1 - l1) / 2; i += PHM_WAVE) {
                d1[3 * i] = M->start[0];
                d1[3 * i + 1] = M->start[1];
                d1[3 * i + 2] = M->start[2];
                ws_m[base + i] = M->start[0];
                ws_x[base + i] = M->start[1];
                ws_y[base + i] = M->start[2];
            }
        }
        lds_barrier();
        for (int d = 1; d <= n; d++) {
            int l, r;
            limits(d, l, r);
            const int width = (r - l) / 2 + 1;
            const int64_t base = cell_first[p.diag0 + d];
            for (int i = lane; i < width; i += PHM_WAVE) {
                const int xmy = l + 2 * i;
                const int x = (d + xmy) >> 1, y = (d - xmy) >> 1;
                St lower{PHM_NEG, PHM_NEG, PHM_NEG}, middle = lower, upper = lower;
                if (xmy - 1 >= l1 && xmy - 1 <= r1) { const double *c = d1 + 3 * ((xmy - 1 - l1) >> 1); lower = St{c[0], c[1], c[2]}; }
                if (xmy + 1 >= l1 && xmy + 1 <= r1) { const double *c = d1 + 3 * ((xmy + 1 - l1) >> 1); upper = St{c[0], c[1], c[2]}; }
                if (xmy >= l2 && xmy <= r2) { const double *c = d2 + 3 * ((xmy - l2) >> 1); middle = St{c[0], c[1], c[2]}; }
                int cx = 4, cy = 4;
                if (x > 0) cx = pst_sym(sx, x - 1);
                if (y > 0) cy = pst_sym(sy, y - 1);
                const double eY = M->ey[cy];
                const PhmRowT ty{eY + t[4], eY + t[6], eY + t[8]};
                const St cur = phm_cell(lower, middle, upper, t, M->ex[cx], M->em[cx * 5 + cy], ty);
                d0[3 * i] = cur.m;
                d0[3 * i + 1] = cur.x;
                d0[3 * i + 2] = cur.y;
                ws_m[base + i] = cur.m;
                ws_x[base + i] = cur.x;
                ws_y[base + i] = cur.y;
            }
            lds_barrier();
            double *tmp = d2;
            d2 = d1; d1 = d0; d0 = tmp;
            l2 = l1; r2 = r1; l1 = l; r1 = r;
        }
        lds_barrier();
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

/* One traceback of one pair (pairwiseAligner.c:752-829), a wave.  b0 / b1 / b2: the backward diagonals d', d' + 1, d' + 2.
 *
 * The reference's diagonalCalculationBackward at diagonal d2 lets every cell of d2, ascending in x - y, push into its lower and upper
 * neighbour on d2 - 1 and into its middle one on d2 - 2.  Seen from the cell (d', z) that receives, in the order of arrival: the match
 * transition of (d' + 2, z), pushed while d' + 2 was walked; then, while d' + 1 is walked, the gap-y transition of (d' + 1, z - 1),
 * whose `upper` this cell is; then the gap-x transition of (d' + 1, z + 1), whose `lower` it is.  A state of the receiving cell gets one
 * term from each, b_successor[to] + (eP + tP) with the successor's symbols; a successor outside the band or beyond d gives none. */
__global__ void __launch_bounds__(PHM_WAVE) pst_traceback_kernel(const PstPair *__restrict__ pairs, const PstTb *__restrict__ tbs,
                                                                   const uint8_t *__restrict__ pool, const PhmModelDev *__restrict__ models,
                                                                   const int32_t *__restrict__ band, const int64_t *__restrict__ cell_first, int W,
                                                                   const double *__restrict__ ws_m, const double *__restrict__ ws_x,
                                                                   const double *__restrict__ ws_y, double cut, int with_gaps, int ragged_right,
                                                                   int64_t n_tb_group, PstCand *__restrict__ cand_m, PstCand *__restrict__ cand_x,
                                                                   PstCand *__restrict__ cand_y, int32_t *__restrict__ counts,
                                                                   double *__restrict__ total_out) {
    extern __shared__ double pst_lds[]; /* 3 diagonals x W cells x 3 states */
    const int lane = threadIdx.x;
    const PstTb tb = tbs[blockIdx.x];
    const PstPair p = pairs[tb.pair];
    const int lx = p.lx, ly = p.ly, n = lx + ly;
    const PhmModelDev *__restrict__ M = models + p.model;
    double t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = M->t[i];
    const uint8_t *__restrict__ sx = pool + p.x_off;
    const uint8_t *__restrict__ sy = pool + p.y_off;
    const int32_t *__restrict__ bnd = band + 2 * p.diag0;
    const int64_t *__restrict__ first = cell_first + p.diag0;
    const int d = tb.d;
    const bool at_end = d == n;
    /* the end state probabilities, ragged only at the end of the matrix (:754-756, stateMachine.c:532-560) */
    double e_end[3];
    if (at_end && ragged_right) {
        e_end[0] = (t[3] + t[4]) / 2.0;
        e_end[1] = t[5];
        e_end[2] = t[6];
    } else {
        e_end[0] = t[0];
        e_end[1] = t[1];
        e_end[2] = t[2];
    }
    double *b0 = pst_lds, *b1 = pst_lds + 3 * W, *b2 = pst_lds + 6 * W;
    int l1 = 1, r1 = 0, l2 = 1, r2 = 0; /* the limits of d' + 1 and d' + 2: empty beyond d */
    PstCand *__restrict__ list_m = cand_m + tb.cand_base;
    PstCand *__restrict__ list_x = with_gaps ? cand_x + tb.cand_base : nullptr;
    PstCand *__restrict__ list_y = with_gaps ? cand_y + tb.cand_base : nullptr;
    int n_m = 0, n_x = 0, n_y = 0;
    int taken = 0; /* totalPosteriorCalculationsThisTraceback */
    double total = PHM_NEG;
    for (int dd = d; dd > tb.to; dd--) {
        const int l0 = bnd[2 * dd], r0 = bnd[2 * dd + 1];
        const int width = (r0 - l0) / 2 + 1;
        if (dd == d) {
            for (int i = lane; i < width; i += PHM_WAVE) {
                b0[3 * i] = e_end[0];
                b0[3 * i + 1] = e_end[1];
                b0[3 * i + 2] = e_end[2];
            }
        } else {
            for (int i = lane; i < width; i += PHM_WAVE) {
                const int z = l0 + 2 * i;
                const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                St b{PHM_NEG, PHM_NEG, PHM_NEG};
                if (z >= l2 && z <= r2) { /* (x + 1, y + 1) */
                    const double sm = b2[3 * ((z - l2) >> 1)];
                    const double eM = M->em[pst_sym(sx, x) * 5 + pst_sym(sy, y)];
                    b.m = phm_log_add(b.m, sm + (eM + t[0]));
                    b.x = phm_log_add(b.x, sm + (eM + t[1]));
                    b.y = phm_log_add(b.y, sm + (eM + t[2]));
                }
                if (z - 1 >= l1 && z - 1 <= r1) { /* (x, y + 1) */
                    const double s_y = b1[3 * ((z - 1 - l1) >> 1) + 2];
                    const double eY = M->ey[pst_sym(sy, y)];
                    b.m = phm_log_add(b.m, s_y + (eY + t[4]));
                    b.y = phm_log_add(b.y, s_y + (eY + t[6]));
                    b.x = phm_log_add(b.x, s_y + (eY + t[8]));
                }
                if (z + 1 >= l1 && z + 1 <= r1) { /* (x + 1, y) */
                    const double s_x = b1[3 * ((z + 1 - l1) >> 1) + 1];
                    const double eX = M->ex[pst_sym(sx, x)];
                    b.m = phm_log_add(b.m, s_x + (eX + t[3]));
                    b.x = phm_log_add(b.x, s_x + (eX + t[5]));
                    b.y = phm_log_add(b.y, s_x + (eX + t[7]));
                }
                b0[3 * i] = b.m;
                b0[3 * i + 1] = b.x;
                b0[3 * i + 2] = b.y;
            }
        }
        lds_barrier();
        if (dd <= tb.from) {
            const int64_t base = first[dd];
            if (taken % 10 == 0) {
                /* diagonalCalculationTotalProbability (:578-596).  b2 is dead from here until the next diagonal is written into it:
                 * its first W doubles take the cells' terms of the first dot product, the next W those of the second */
                double *term = b2;
                for (int i = lane; i < width; i += PHM_WAVE) {
                    const double bb[3] = {b0[3 * i], b0[3 * i + 1], b0[3 * i + 2]};
                    term[i] = phm_dot(St{ws_m[base + i], ws_x[base + i], ws_y[base + i]}, bb);
                }
                const bool second = dd < d; /* diagonal dd + 1 has a backward diagonal; the forward diagonal dd - 1 always exists */
                const int width1 = second ? (r1 - l1) / 2 + 1 : 0;
                if (second) {
                    const int lm = bnd[2 * (dd - 1)], rm = bnd[2 * (dd - 1) + 1];
                    const int64_t base_m = first[dd - 1];
                    for (int j = lane; j < width1; j += PHM_WAVE) {
                        /* the match state of a forward step from diagonal dd - 1 onto the cell of dd + 1; its gap states stay LOG_ZERO */
                        const int z = l1 + 2 * j;
                        const int x = (dd + 1 + z) >> 1, y = (dd + 1 - z) >> 1;
                        St mid{PHM_NEG, PHM_NEG, PHM_NEG};
                        if (z >= lm && z <= rm) {
                            const int64_t c = base_m + ((z - lm) >> 1);
                            mid = St{ws_m[c], ws_x[c], ws_y[c]};
                        }
                        int cx = 4, cy = 4;
                        if (x > 0) cx = pst_sym(sx, x - 1);
                        if (y > 0) cy = pst_sym(sy, y - 1);
                        const double eM = M->em[cx * 5 + cy];
                        const St f{phm_chain(mid.m + (eM + t[0]), mid.x + (eM + t[1]), mid.y + (eM + t[2])), PHM_NEG, PHM_NEG};
                        const double bb[3] = {b1[3 * j], b1[3 * j + 1], b1[3 * j + 2]};
                        term[W + j] = phm_dot(f, bb);
                    }
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
                    if (dd == n) total_out[p.slot] = tot;
                }
                lds_barrier();
                total = term[2 * W];
            }
            taken++;
            /* diagonalCalculationPosteriorMatchProbs / ...PosteriorProbs (:610-681), ascending in x - y */
            for (int c0 = 0; c0 < width; c0 += PHM_WAVE) {
                const int i = c0 + lane;
                const bool in = i < width;
                const int z = l0 + 2 * (in ? i : 0);
                const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                const int64_t c = base + (in ? i : 0);
                const int k = 3 * (in ? i : 0);
                const double vm = (ws_m[c] + b0[k]) - total;
                pst_emit(list_m, n_m, in && x > 0 && y > 0 && vm >= cut, x - 1, y - 1, vm);
                if (with_gaps) {
                    const double vx = (ws_x[c] + b0[k + 1]) - total;
                    pst_emit(list_x, n_x, in && x > 0 && vx >= cut, x - 1, y - 1, vx);
                    const double vy = (ws_y[c] + b0[k + 2]) - total;
                    pst_emit(list_y, n_y, in && y > 0 && vy >= cut, x - 1, y - 1, vy);
                }
            }
        }
        lds_barrier(); /* every read of b2 (the terms, the total) is done before it is written as the next b0 */
        double *tmp = b2;
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
template <int T>
__global__ void __launch_bounds__(T) pst_forward_wide_kernel(const PstPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                             const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band,
                                                             const int64_t *__restrict__ cell_first, double *ws_m, double *ws_x, double *ws_y) {
    const int tid = threadIdx.x;
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PstPair p = pairs[pi];
        const int n = p.lx + p.ly;
        const PhmModelDev *__restrict__ M = models + p.model;
        double t[9];
#pragma unroll
        for (int i = 0; i < 9; i++) t[i] = M->t[i];
        const uint8_t *__restrict__ sx = pool + p.x_off;
        const uint8_t *__restrict__ sy = pool + p.y_off;
        const int32_t *__restrict__ bnd = band + 2 * p.diag0;
        const int64_t *__restrict__ first = cell_first + p.diag0;
        int l1 = bnd[0], r1 = bnd[1], l2 = 1, r2 = 0; /* the limits of xay - 1 and xay - 2 */
        int64_t base1 = first[0], base2 = 0;          /* and their first cells */
        for (int i = tid; i <= (r1 - l1) / 2; i += T) {
            ws_m[base1 + i] = M->start[0];
            ws_x[base1 + i] = M->start[1];
            ws_y[base1 + i] = M->start[2];
        }
        __syncthreads();
        for (int d = 1; d <= n; d++) {
            const int l = bnd[2 * d], r = bnd[2 * d + 1];
            const int width = (r - l) / 2 + 1;
            const int64_t base = first[d];
            for (int i = tid; i < width; i += T) {
                const int xmy = l + 2 * i;
                const int x = (d + xmy) >> 1, y = (d - xmy) >> 1;
                St lower{PHM_NEG, PHM_NEG, PHM_NEG}, middle = lower, upper = lower;
                if (xmy - 1 >= l1 && xmy - 1 <= r1) { const int64_t c = base1 + ((xmy - 1 - l1) >> 1); lower = St{ws_m[c], ws_x[c], ws_y[c]}; }
                if (xmy + 1 >= l1 && xmy + 1 <= r1) { const int64_t c = base1 + ((xmy + 1 - l1) >> 1); upper = St{ws_m[c], ws_x[c], ws_y[c]}; }
                if (xmy >= l2 && xmy <= r2) { const int64_t c = base2 + ((xmy - l2) >> 1); middle = St{ws_m[c], ws_x[c], ws_y[c]}; }
                int cx = 4, cy = 4;
                if (x > 0) cx = pst_sym(sx, x - 1);
                if (y > 0) cy = pst_sym(sy, y - 1);
                const double eY = M->ey[cy];
                const PhmRowT ty{eY + t[4], eY + t[6], eY + t[8]};
                const St cur = phm_cell(lower, middle, upper, t, M->ex[cx], M->em[cx * 5 + cy], ty);
                ws_m[base + i] = cur.m;
                ws_x[base + i] = cur.x;
                ws_y[base + i] = cur.y;
            }
            __syncthreads();
            l2 = l1; r2 = r1; base2 = base1;
            l1 = l; r1 = r; base1 = base;
        }
    }
}

/* pst_traceback_kernel with a (pair, traceback) per workgroup, grid-stride over the launch's tracebacks.  The workgroup's slice of a
 * second workspace, 11 * W doubles (W: the widest diagonal of the launch): the backward diagonals d', d' + 1, d' + 2 as
 * [diagonal][state][W], rotating by pointer, and the two rows of the total's terms.  The gather of a cell is
 * pst_traceback_kernel's, term for term.  The totals are folded serially, ascending in x - y, by the first wave (below).
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

template <int T>
__global__ void __launch_bounds__(T) pst_traceback_wide_kernel(const PstPair *__restrict__ pairs, const PstTb *__restrict__ tbs, int64_t n_tbs,
                                                               const uint8_t *__restrict__ pool, const PhmModelDev *__restrict__ models,
                                                               const int32_t *__restrict__ band, const int64_t *__restrict__ cell_first, int W,
                                                               const double *__restrict__ ws_m, const double *__restrict__ ws_x,
                                                               const double *__restrict__ ws_y, double *ws_back, double cut, int with_gaps,
                                                               int ragged_right, int64_t n_tb_group, PstCand *__restrict__ cand_m,
                                                               PstCand *__restrict__ cand_x, PstCand *__restrict__ cand_y,
                                                               int32_t *__restrict__ counts, double *__restrict__ total_out) {
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
        const PstPair p = pairs[tb.pair];
        const int n = p.lx + p.ly;
        const PhmModelDev *__restrict__ M = models + p.model;
        double t[9];
#pragma unroll
        for (int i = 0; i < 9; i++) t[i] = M->t[i];
        const uint8_t *__restrict__ sx = pool + p.x_off;
        const uint8_t *__restrict__ sy = pool + p.y_off;
        const int32_t *__restrict__ bnd = band + 2 * p.diag0;
        const int64_t *__restrict__ first = cell_first + p.diag0;
        const int d = tb.d;
        const bool at_end = d == n;
        double e_end[3]; /* ragged only at the end of the matrix (:754-756, stateMachine.c:532-560) */
        if (at_end && ragged_right) {
            e_end[0] = (t[3] + t[4]) / 2.0;
            e_end[1] = t[5];
            e_end[2] = t[6];
        } else {
            e_end[0] = t[0];
            e_end[1] = t[1];
            e_end[2] = t[2];
        }
        double *b0 = slice, *b1 = slice + 3 * (size_t) W, *b2 = slice + 6 * (size_t) W;
        int l1 = 1, r1 = 0, l2 = 1, r2 = 0; /* the limits of d' + 1 and d' + 2: empty beyond d */
        PstCand *__restrict__ list_m = cand_m + tb.cand_base;
        PstCand *__restrict__ list_x = with_gaps ? cand_x + tb.cand_base : nullptr;
        PstCand *__restrict__ list_y = with_gaps ? cand_y + tb.cand_base : nullptr;
        int n_m = 0, n_x = 0, n_y = 0;
        int taken = 0; /* totalPosteriorCalculationsThisTraceback */
        double total = PHM_NEG;
        for (int dd = d; dd > tb.to; dd--) {
            const int l0 = bnd[2 * dd], r0 = bnd[2 * dd + 1];
            const int width = (r0 - l0) / 2 + 1;
            if (dd == d) {
                for (int i = tid; i < width; i += T) {
                    b0[i] = e_end[0];
                    b0[W + i] = e_end[1];
                    b0[2 * W + i] = e_end[2];
                }
            } else {
                for (int i = tid; i < width; i += T) {
                    const int z = l0 + 2 * i;
                    const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                    St b{PHM_NEG, PHM_NEG, PHM_NEG};
                    if (z >= l2 && z <= r2) { /* (x + 1, y + 1) */
                        const double sm = b2[(z - l2) >> 1];
                        const double eM = M->em[pst_sym(sx, x) * 5 + pst_sym(sy, y)];
                        b.m = phm_log_add(b.m, sm + (eM + t[0]));
                        b.x = phm_log_add(b.x, sm + (eM + t[1]));
                        b.y = phm_log_add(b.y, sm + (eM + t[2]));
                    }
                    if (z - 1 >= l1 && z - 1 <= r1) { /* (x, y + 1) */
                        const double s_y = b1[2 * W + ((z - 1 - l1) >> 1)];
                        const double eY = M->ey[pst_sym(sy, y)];
                        b.m = phm_log_add(b.m, s_y + (eY + t[4]));
                        b.y = phm_log_add(b.y, s_y + (eY + t[6]));
                        b.x = phm_log_add(b.x, s_y + (eY + t[8]));
                    }
                    if (z + 1 >= l1 && z + 1 <= r1) { /* (x + 1, y) */
                        const double s_x = b1[W + ((z + 1 - l1) >> 1)];
                        const double eX = M->ex[pst_sym(sx, x)];
                        b.m = phm_log_add(b.m, s_x + (eX + t[3]));
                        b.x = phm_log_add(b.x, s_x + (eX + t[5]));
                        b.y = phm_log_add(b.y, s_x + (eX + t[7]));
                    }
                    b0[i] = b.m;
                    b0[W + i] = b.x;
                    b0[2 * W + i] = b.y;
                }
            }
            __syncthreads();
            if (dd <= tb.from) {
                const int64_t base = first[dd];
                if (taken % 10 == 0) {
                    /* diagonalCalculationTotalProbability (:578-596): the cells' terms side by side, the fold by one thread */
                    for (int i = tid; i < width; i += T) {
                        const double bb[3] = {b0[i], b0[W + i], b0[2 * W + i]};
                        term[i] = phm_dot(St{ws_m[base + i], ws_x[base + i], ws_y[base + i]}, bb);
                    }
                    const bool second = dd < d; /* diagonal dd + 1 has a backward diagonal; the forward diagonal dd - 1 always exists */
                    const int width1 = second ? (r1 - l1) / 2 + 1 : 0;
                    if (second) {
                        const int lm = bnd[2 * (dd - 1)], rm = bnd[2 * (dd - 1) + 1];
                        const int64_t base_m = first[dd - 1];
                        for (int j = tid; j < width1; j += T) {
                            /* the match state of a forward step from diagonal dd - 1 onto the cell of dd + 1; its gap states stay LOG_ZERO */
                            const int z = l1 + 2 * j;
                            const int x = (dd + 1 + z) >> 1, y = (dd + 1 - z) >> 1;
                            St mid{PHM_NEG, PHM_NEG, PHM_NEG};
                            if (z >= lm && z <= rm) {
                                const int64_t c = base_m + ((z - lm) >> 1);
                                mid = St{ws_m[c], ws_x[c], ws_y[c]};
                            }
                            int cx = 4, cy = 4;
                            if (x > 0) cx = pst_sym(sx, x - 1);
                            if (y > 0) cy = pst_sym(sy, y - 1);
                            const double eM = M->em[cx * 5 + cy];
                            const St f{phm_chain(mid.m + (eM + t[0]), mid.x + (eM + t[1]), mid.y + (eM + t[2])), PHM_NEG, PHM_NEG};
                            const double bb[3] = {b1[j], b1[W + j], b1[2 * W + j]};
                            term[W + j] = phm_dot(f, bb);
                        }
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
                    if (tid == 0 && dd == n) total_out[p.slot] = total;
                }
                taken++;
                /* diagonalCalculationPosteriorMatchProbs / ...PosteriorProbs (:610-681), ascending in x - y across the workgroup */
                for (int c0 = 0; c0 < width; c0 += T) {
                    const int i = c0 + tid;
                    const bool in = i < width;
                    const int ii = in ? i : 0;
                    const int z = l0 + 2 * ii;
                    const int x = (dd + z) >> 1, y = (dd - z) >> 1;
                    const int64_t c = base + ii;
                    const double vm = (ws_m[c] + b0[ii]) - total;
                    const double vx = with_gaps ? (ws_x[c] + b0[W + ii]) - total : PHM_NEG;
                    const double vy = with_gaps ? (ws_y[c] + b0[2 * W + ii]) - total : PHM_NEG;
                    const bool keep_m = in && x > 0 && y > 0 && vm >= cut;
                    const bool keep_x = with_gaps && in && x > 0 && vx >= cut;
                    const bool keep_y = with_gaps && in && y > 0 && vy >= cut;
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
            double *tmp = b2;
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

/* What the host knows of a pair before anything is launched */
struct PstHostPair {
    int64_t band_first; /* its diagonal 0 in the call's band arrays */
    int64_t cells;
    int64_t tb_first;   /* its tracebacks in the call's plan */
    int32_t width;
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

/* The two entries.  dynamic: the band is band_constructDynamic's over anchor_expansion (one per anchor, indexed as the anchors are);
 * else band_construct's over opt->expansion.  Everything behind the band is the same call. */
static int pst_aligned_pairs(const char *who, bool dynamic, mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, int64_t n_pairs,
                             const uint8_t *pool, int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len, const int64_t *y_off,
                             const int32_t *y_len, const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors,
                             const int64_t *anchor_expansion, const mrp_posterior_options *opt, mrp_posterior_pairs *match_out,
                             mrp_posterior_pairs *gap_x_out, mrp_posterior_pairs *gap_y_out, double *total_out, mrp_pairhmm_stats *stats) {
    const double t_begin = now_ms();
    /* ---- MRP_ERR_ARG ---- */
    if (!models || !opt || !match_out || n_models <= 0 || n_pairs < 0 || pool_bytes < 0 || (pool_bytes > 0 && !pool))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (n_pairs > 0 && (!x_off || !x_len || !y_off || !y_len)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    if (const char *msg = pst_options_error(opt)) return mrp_set_error(MRP_ERR_ARG, "%s: %s", who, msg);
    if (opt->with_gaps != 0 && opt->with_gaps != 1) return mrp_set_error(MRP_ERR_ARG, "%s: with_gaps must be 0 or 1", who);
    if ((opt->with_gaps != 0) != (gap_x_out != nullptr) || (opt->with_gaps != 0) != (gap_y_out != nullptr))
        return mrp_set_error(MRP_ERR_ARG, "%s: gap_x_out and gap_y_out must be given exactly when with_gaps is set", who);
    for (int64_t i = 0; i < n_pairs; i++) {
        const int64_t lx = x_len[i], ly = y_len[i];
        const int64_t na = anchor_off ? anchor_off[i + 1] - anchor_off[i] : 0;
        if (lx < 0 || ly < 0 || x_off[i] < 0 || y_off[i] < 0 || x_off[i] + lx > pool_bytes || y_off[i] + ly > pool_bytes ||
            (anchor_off && anchor_off[i] < 0) || na < 0 || (na > 0 && (!anchors || (dynamic && !anchor_expansion))))
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld lies outside the symbol pool or has bad anchor offsets", who, (long long) i);
        if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld: strings too long", who, (long long) i);
    }
    for (int64_t i = 0; i < n_pairs; i++)
        if (model_index && model_index[i] >= n_models)
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld names model %d of %d", who, (long long) i, (int) model_index[i], (int) n_models);
    /* the bands (band_construct, :175-226, or band_constructDynamic, :120-173) and, from them alone, the tracebacks */
    std::vector<PstHostPair> hp((size_t) n_pairs);
    std::vector<int32_t> Lb, Rb;
    std::vector<PstTraceback> plan;
    int64_t n_diags = 0, cells_all = 0;
    for (int64_t i = 0; i < n_pairs; i++) {
        const int64_t lx = x_len[i], ly = y_len[i], n = lx + ly;
        const int64_t na = anchor_off ? anchor_off[i + 1] - anchor_off[i] : 0;
        Lb.resize((size_t) (n_diags + n + 1));
        Rb.resize((size_t) (n_diags + n + 1));
        PstHostPair &h = hp[(size_t) i];
        h.band_first = n_diags;
        int width = 1;
        if (band_closed_form_any(na > 0 ? anchors + 2 * anchor_off[i] : nullptr, dynamic && na > 0 ? anchor_expansion + anchor_off[i] : nullptr, dynamic, na, lx, ly,
                                 opt->expansion, Lb.data() + n_diags, Rb.data() + n_diags, &h.cells, &width) != MRP_OK)
            return mrp_set_error(MRP_ERR_ARG, dynamic ? "%s: pair %lld has invalid anchors or an odd or negative anchor expansion (pairwiseAligner.c:151-158)"
                                                      : "%s: pair %lld has invalid anchors (pairwiseAligner.c:206-211)",
                                 who, (long long) i);
        h.width = width;
        h.tb_first = (int64_t) plan.size();
        pst_plan_tracebacks(Lb.data() + n_diags, Rb.data() + n_diags, n, opt->expansion, opt->min_diags_between_traceback, opt->traceback_diagonals, plan);
        n_diags += n + 1;
        cells_all += h.cells;
    }
    /* ---- MRP_ERR_UNSUPPORTED ---- */
    const int64_t budget = ctx && ctx->posterior_workspace > 0 ? ctx->posterior_workspace : PST_DEFAULT_WORKSPACE;
    const bool wide_on = ctx && ctx->posterior_wide_pairs;
    for (int64_t i = 0; i < n_pairs; i++) {
        if (hp[(size_t) i].width <= PHM_WAVE_MAX_WIDTH) continue;
        if (!wide_on)
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d; wide pairs are not extended to this entry)", who,
                                 (long long) i, (int) hp[(size_t) i].width, PHM_WAVE_MAX_WIDTH);
        if (hp[(size_t) i].width > MRP_WIDE_MAX_WIDTH)
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d with posterior wide pairs on, MRP_WIDE_MAX_WIDTH)", who,
                                 (long long) i, (int) hp[(size_t) i].width, (int) MRP_WIDE_MAX_WIDTH);
    }
    for (int64_t i = 0; i < n_pairs; i++)
        if (hp[(size_t) i].cells * PST_CELL_BYTES > budget)
            return mrp_set_error(MRP_ERR_UNSUPPORTED,
                                 "%s: pair %lld keeps %lld band cells, %lld bytes of forward diagonals (limit %lld bytes, mrp_context_set_posterior_workspace)", who,
                                 (long long) i, (long long) hp[(size_t) i].cells, (long long) (hp[(size_t) i].cells * PST_CELL_BYTES), (long long) budget);
    for (int64_t i = 0; i < n_pairs; i++) /* (a traceback counts its candidates in 32 bits) */
        if (hp[(size_t) i].cells >= (1ll << 31))
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld keeps %lld band cells (limit 2^31 - 1 whatever the workspace)", who, (long long) i,
                                 (long long) hp[(size_t) i].cells);
    /* ---- MRP_ERR_NO_DEVICE ---- */
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the pair-HMM path has no CPU fallback)", who);

    const int n_lists = opt->with_gaps ? 3 : 1;
    const double cut = log(opt->threshold) - 1e-6; /* wider than the rule by far more than exp() errs: the host decides */
    PstList lists[3];
    std::vector<double> totals((size_t) n_pairs, 0.0);
    mrp_posterior_stats ps;
    memset(&ps, 0, sizeof(ps));
    ps.cells = cells_all;
    std::vector<PhmModelDev> hm((size_t) n_models);
    for (int i = 0; i < n_models; i++) model_to_device(models[i], opt->ragged_left != 0, opt->ragged_right != 0, hm[(size_t) i]);
    int64_t n_scored = 0;
    if (n_pairs > 0) {
        PHM_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        static PerDeviceOnce once;
        const hipError_t configured = once.run([] {
            hipError_t e = hipFuncSetAttribute((const void *) pst_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * PHM_WAVE_MAX_WIDTH * (int) sizeof(double));
            if (e == hipSuccess)
                e = hipFuncSetAttribute((const void *) pst_traceback_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * PHM_WAVE_MAX_WIDTH * (int) sizeof(double));
            return e;
        });
        PHM_HIP(configured);
        DevBuf<PhmModelDev> d_models;
        DevBuf<uint8_t> d_pool;
        d_models.pool = d_pool.pool = &ctx->pool;
        Drain drain{s};
        PHM_HIP(d_models.upload(hm, s));
        PHM_HIP(d_pool.alloc((size_t) pool_bytes));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));

        /* the groups: consecutive pairs whose forward diagonals fit the workspace together */
        /* launch classes 0..3: the pair-per-wave kernels by LDS; class 4: the pair-per-workgroup kernels.  Test hook bit 7 sends every
         * pair there, at PST_WIDE_HOOK_THREADS and a grid of one workgroup, so that consecutive pairs and tracebacks reuse one slice */
        const bool wide_hook = (ctx->test_hooks & 128) != 0;
        HostVec<PstPair> g_pairs[5];
        HostVec<PstTb> g_tbs[5];
        HostVec<int32_t> g_band;
        HostVec<int64_t> g_cell_first, g_cand_base, g_dense_first;
        HostVec<int32_t> g_counts;
        HostVec<PstCand> g_dense;
        HostVec<double> g_total;
        for (int64_t g0 = 0; g0 < n_pairs;) {
            int64_t g1 = g0, g_cells = 0;
            while (g1 < n_pairs && (g1 == g0 || (g_cells + hp[(size_t) g1].cells) * PST_CELL_BYTES <= budget)) g_cells += hp[(size_t) g1++].cells;
            /* host half of the group */
            for (int c = 0; c < 5; c++) { g_pairs[c].clear(); g_tbs[c].clear(); }
            int wide_width = 1;       /* the widest diagonal of class 4 */
            int64_t wide_cells = 0;   /* its band cells */
            g_band.clear();
            g_cell_first.clear();
            g_cand_base.clear();
            int64_t cell = 0, cand = 0, n_tb = 0, n_slot = 0;
            std::vector<int64_t> tb_slot0((size_t) (g1 - g0), -1), pair_slot((size_t) (g1 - g0), -1);
            for (int64_t i = g0; i < g1; i++) {
                const PstHostPair &h = hp[(size_t) i];
                const int64_t n = (int64_t) x_len[i] + y_len[i];
                if (n == 0) continue; /* two empty strings: no lists, a total of 0.0 (:721-723) */
                int c = 0;
                if (wide_hook || h.width > PHM_WAVE_MAX_WIDTH) {
                    c = 4;
                    wide_width = std::max(wide_width, (int) h.width);
                    wide_cells += h.cells;
                } else {
                    while (h.width > WAVE_CLASS_CAP[c]) c++;
                }
                PstPair p;
                p.x_off = x_off[i];
                p.y_off = y_off[i];
                p.diag0 = (int64_t) g_cell_first.size();
                p.lx = x_len[i];
                p.ly = y_len[i];
                p.model = model_index ? model_index[i] : 0;
                p.slot = (int32_t) n_slot;
                pair_slot[(size_t) (i - g0)] = n_slot++;
                for (int64_t d = 0; d <= n; d++) {
                    const int32_t l = Lb[(size_t) (h.band_first + d)], r = Rb[(size_t) (h.band_first + d)];
                    g_band.push_back(l);
                    g_band.push_back(r);
                    g_cell_first.push_back(cell);
                    cell += (r - l) / 2 + 1;
                }
                const int64_t tb_end = i + 1 < n_pairs ? hp[(size_t) i + 1].tb_first : (int64_t) plan.size();
                tb_slot0[(size_t) (i - g0)] = n_tb;
                for (int64_t k = h.tb_first; k < tb_end; k++) {
                    const PstTraceback &q = plan[(size_t) k];
                    PstTb tb;
                    tb.pair = (int32_t) g_pairs[c].size();
                    tb.d = (int32_t) q.d;
                    tb.to = (int32_t) q.to;
                    tb.from = (int32_t) q.from;
                    tb.slot = n_tb++;
                    tb.cand_base = cand;
                    g_cand_base.push_back(cand);
                    /* at most one candidate per list and cell of the diagonals (to, from] */
                    cand += g_cell_first[(size_t) (p.diag0 + q.from)] + (Rb[(size_t) (h.band_first + q.from)] - Lb[(size_t) (h.band_first + q.from)]) / 2 + 1 -
                            g_cell_first[(size_t) (p.diag0 + q.to + 1)];
                    ps.traceback_cells += g_cell_first[(size_t) (p.diag0 + q.d)] + (Rb[(size_t) (h.band_first + q.d)] - Lb[(size_t) (h.band_first + q.d)]) / 2 + 1 -
                                          g_cell_first[(size_t) (p.diag0 + q.to + 1)];
                    g_tbs[c].push_back(tb);
                }
                g_pairs[c].push_back(p);
            }
            ps.groups++;
            n_scored += n_slot;
            if (n_slot > 0) {
                PstGroupDev G;
                G.arrays.bind(&ctx->pool);
                G.s = s;
                /* one array of pairs and one of tracebacks, class after class */
                HostVec<PstPair> all_pairs;
                HostVec<PstTb> all_tbs;
                int64_t pair0[6] = {0, 0, 0, 0, 0, 0}, tb0[6] = {0, 0, 0, 0, 0, 0};
                for (int c = 0; c < 5; c++) {
                    all_pairs.insert(all_pairs.end(), g_pairs[c].begin(), g_pairs[c].end());
                    all_tbs.insert(all_tbs.end(), g_tbs[c].begin(), g_tbs[c].end());
                    pair0[c + 1] = (int64_t) all_pairs.size();
                    tb0[c + 1] = (int64_t) all_tbs.size();
                }
                PHM_HIP(G.d_pairs.upload(all_pairs, s));
                PHM_HIP(G.d_tbs.upload(all_tbs, s));
                PHM_HIP(G.d_band.upload(g_band, s));
                PHM_HIP(G.d_cell_first.upload(g_cell_first, s));
                PHM_HIP(G.d_cand_base.upload(g_cand_base, s));
                PHM_HIP(G.d_ws.alloc(3 * (size_t) cell));
                PHM_HIP(G.d_cand.alloc((size_t) n_lists * (size_t) cand));
                PHM_HIP(G.d_counts.alloc(3 * (size_t) n_tb));
                PHM_HIP(G.d_total.alloc((size_t) n_slot));
                double *ws_m = G.d_ws.p, *ws_x = G.d_ws.p + cell, *ws_y = G.d_ws.p + 2 * cell;
                /* class 4: a slice of backward diagonals per workgroup of the traceback kernel, as many as PHM_WIDE_WORKSPACE_BYTES holds */
                const int64_t n_wide = pair0[5] - pair0[4], n_wide_tb = tb0[5] - tb0[4];
                const int64_t slice_doubles = 11 * (int64_t) wide_width;
                const int64_t wide_fgrid = wide_hook ? 1 : std::min<int64_t>(n_wide, 1 << 20);
                const int64_t wide_tgrid =
                    wide_hook ? 1 : std::min<int64_t>(n_wide_tb, std::max<int64_t>(1, PHM_WIDE_WORKSPACE_BYTES / (slice_doubles * (int64_t) sizeof(double))));
                if (n_wide_tb > 0) PHM_HIP(G.d_ws_back.alloc((size_t) (wide_tgrid * slice_doubles)));
                PHM_HIP(hipStreamSynchronize(s)); /* the uploads are not part of the kernels' time */
                PHM_HIP(hipEventRecord(ctx->ev[0], s));
                for (int c = 0; c < 4; c++) {
                    const int64_t n = pair0[c + 1] - pair0[c];
                    if (n == 0) continue;
                    const int W = WAVE_CLASS_CAP[c];
                    hipLaunchKernelGGL(pst_forward_kernel, dim3((unsigned) std::min<int64_t>(n, 1 << 20)), dim3(PHM_WAVE), (size_t) 9 * W * sizeof(double), s,
                                       G.d_pairs.p + pair0[c], n, d_pool.p, d_models.p, G.d_band.p, G.d_cell_first.p, W, ws_m, ws_x, ws_y);
                    PHM_HIP(hipGetLastError());
                }
                if (n_wide > 0) {
                    auto launch = [&](auto threads) {
                        constexpr int T = decltype(threads)::value;
                        hipLaunchKernelGGL((pst_forward_wide_kernel<T>), dim3((unsigned) wide_fgrid), dim3(T), 0, s, G.d_pairs.p + pair0[4], n_wide, d_pool.p, d_models.p,
                                           G.d_band.p, G.d_cell_first.p, ws_m, ws_x, ws_y);
                    };
                    if (wide_hook) launch(std::integral_constant<int, PST_WIDE_HOOK_THREADS>{});
                    else launch(std::integral_constant<int, PST_WIDE_THREADS>{});
                    PHM_HIP(hipGetLastError());
                }
                PHM_HIP(hipEventRecord(ctx->ev[1], s));
                for (int c = 0; c < 4; c++) {
                    const int64_t n = tb0[c + 1] - tb0[c];
                    if (n == 0) continue;
                    const int W = WAVE_CLASS_CAP[c];
                    hipLaunchKernelGGL(pst_traceback_kernel, dim3((unsigned) n), dim3(PHM_WAVE), (size_t) 9 * W * sizeof(double), s, G.d_pairs.p + pair0[c],
                                       G.d_tbs.p + tb0[c], d_pool.p, d_models.p, G.d_band.p, G.d_cell_first.p, W, ws_m, ws_x, ws_y, cut, (int) opt->with_gaps,
                                       (int) (opt->ragged_right != 0), n_tb, G.d_cand.p, G.d_cand.p + cand, G.d_cand.p + 2 * cand, G.d_counts.p, G.d_total.p);
                    PHM_HIP(hipGetLastError());
                }
                if (n_wide_tb > 0) {
                    auto launch = [&](auto threads) {
                        constexpr int T = decltype(threads)::value;
                        hipLaunchKernelGGL((pst_traceback_wide_kernel<T>), dim3((unsigned) wide_tgrid), dim3(T), 0, s, G.d_pairs.p + pair0[4], G.d_tbs.p + tb0[4],
                                           n_wide_tb, d_pool.p, d_models.p, G.d_band.p, G.d_cell_first.p, wide_width, ws_m, ws_x, ws_y, G.d_ws_back.p, cut,
                                           (int) opt->with_gaps, (int) (opt->ragged_right != 0), n_tb, G.d_cand.p, G.d_cand.p + cand, G.d_cand.p + 2 * cand,
                                           G.d_counts.p, G.d_total.p);
                    };
                    if (wide_hook) launch(std::integral_constant<int, PST_WIDE_HOOK_THREADS>{});
                    else launch(std::integral_constant<int, PST_WIDE_THREADS>{});
                    PHM_HIP(hipGetLastError());
                }
                ctx->posterior_wide_count += n_wide;
                ctx->posterior_wide_cells += wide_cells;
                PHM_HIP(hipEventRecord(ctx->ev[2], s));
                g_counts.resize(3 * (size_t) n_tb);
                g_total.resize((size_t) n_slot);
                PHM_HIP(hipMemcpyAsync(g_counts.data(), G.d_counts.p, 3 * (size_t) n_tb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                PHM_HIP(hipMemcpyAsync(g_total.data(), G.d_total.p, (size_t) n_slot * sizeof(double), hipMemcpyDeviceToHost, s));
                PHM_HIP(hipStreamSynchronize(s));
                float ms = 0.f;
                PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
                ps.forward_ms += ms;
                PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
                ps.traceback_ms += ms;
                g_dense_first.resize((size_t) n_lists * (size_t) n_tb);
                int64_t n_dense = 0;
                for (int l = 0; l < n_lists; l++)
                    for (int64_t k = 0; k < n_tb; k++) {
                        g_dense_first[(size_t) (l * n_tb + k)] = n_dense;
                        n_dense += g_counts[(size_t) (l * n_tb + k)];
                    }
                g_dense.resize((size_t) n_dense);
                if (n_dense > 0) {
                    PHM_HIP(G.d_dense_first.upload(g_dense_first, s));
                    PHM_HIP(G.d_dense.alloc((size_t) n_dense));
                    hipLaunchKernelGGL(pst_pack_kernel, dim3((unsigned) n_tb, (unsigned) n_lists), dim3(256), 0, s, G.d_cand.p, cand, G.d_cand_base.p, G.d_counts.p,
                                       G.d_dense_first.p, n_tb, G.d_dense.p);
                    PHM_HIP(hipGetLastError());
                    PHM_HIP(hipMemcpyAsync(g_dense.data(), G.d_dense.p, (size_t) n_dense * sizeof(PstCand), hipMemcpyDeviceToHost, s));
                    PHM_HIP(hipStreamSynchronize(s));
                }
                ps.candidates += n_dense;
                ps.downloaded_bytes += n_dense * (int64_t) sizeof(PstCand) + 3 * n_tb * (int64_t) sizeof(int32_t) + n_slot * (int64_t) sizeof(double);
            }
            ctx->pool.reclaim(); /* the group's arrays are idle: the next group takes them */
            /* the host's rule over the candidates, pair by pair in input order, traceback by traceback */
            for (int64_t i = g0; i < g1; i++) {
                const int64_t slot = pair_slot[(size_t) (i - g0)];
                if (slot >= 0) {
                    totals[(size_t) i] = g_total[(size_t) slot];
                    const int64_t tb_end = i + 1 < n_pairs ? hp[(size_t) i + 1].tb_first : (int64_t) plan.size();
                    const int64_t k0 = tb_slot0[(size_t) (i - g0)], k1 = k0 + (tb_end - hp[(size_t) i].tb_first);
                    for (int l = 0; l < n_lists; l++)
                        for (int64_t k = k0; k < k1; k++)
                            pst_apply_rule(g_dense.data() + g_dense_first[(size_t) (l * n_tb + k)], g_counts[(size_t) (l * n_tb + k)], opt->threshold, lists[l]);
                }
                for (int l = 0; l < n_lists; l++) lists[l].first.push_back((int64_t) lists[l].x.size());
            }
            g0 = g1;
        }
    }
    ctx->pool.reclaim();
    /* nothing has been written so far: hand out */
    mrp_posterior_pairs r[3];
    memset(r, 0, sizeof(r));
    for (int l = 0; l < n_lists; l++) {
        const int rc = pst_hand_out(lists[l], &r[l]);
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
        stats->cells = cells_all;
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
    return pst_aligned_pairs("mrp_posterior_aligned_pairs", false, ctx, models, n_models, n_pairs, pool, pool_bytes, x_off, x_len, y_off, y_len, model_index,
                             anchor_off, anchors, nullptr, opt, match_out, gap_x_out, gap_y_out, total_out, stats);
}

int mrp_posterior_aligned_pairs_dynamic(mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, int64_t n_pairs, const uint8_t *pool,
                                        int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len, const int64_t *y_off, const int32_t *y_len,
                                        const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors, const int64_t *anchor_expansion,
                                        const mrp_posterior_options *opt, mrp_posterior_pairs *match_out, mrp_posterior_pairs *gap_x_out,
                                        mrp_posterior_pairs *gap_y_out, double *total_out, mrp_pairhmm_stats *stats) {
    return pst_aligned_pairs("mrp_posterior_aligned_pairs_dynamic", true, ctx, models, n_models, n_pairs, pool, pool_bytes, x_off, x_len, y_off, y_len,
                             model_index, anchor_off, anchors, anchor_expansion, opt, match_out, gap_x_out, gap_y_out, total_out, stats);
}

}  // extern "C"
