/*
 * mrp_pairhmm_walk.h -- what the banded pair-HMM kernels share, each stated once: the walk over the x+y diagonals of a band
 * (mrp_pairhmm.hip: phm_wave_kernel, phm_wide_kernel; mrp_posterior.hip: pst_forward_kernel, pst_forward_wide_kernel) and the cell
 * arithmetic of a traceback (pst_traceback_kernel, pst_traceback_wide_kernel).  phm_log_add is an interpolation and not associative:
 * the order of its terms is part of the result, so the kernels differ only in who strides over a diagonal's cells and where the
 * diagonals lie.  Device code only; every unit that includes it is compiled with -ffp-contract=off.
 *
 *   one walk       phm_forward_walk: the start diagonal, then diagonal after diagonal from the two before it, a barrier after each
 *   two teams      T threads with __syncthreads (phm_wave_kernel's one wave too, as ever), or a wave with the LDS-only lds_barrier
 *   three storages three rotating buffers; the same with every cell also kept in the workspace; the kept workspace alone (PhmKeep)
 *   two emissions  the match emission of a cell is a policy of the pair's context: the model's table (PhmNucleotide, the default, which
 *                  costs the kernels nothing) or the same + the repeat counts' term from a table in device memory (PhmRunLength,
 *                  DESIGN.md 9.16); the three places that take a match emission -- the forward cell, the match branch of the backward
 *                  cell, the second term of a total -- ask the policy
 */
#ifndef MRP_PAIRHMM_WALK_H_
#define MRP_PAIRHMM_WALK_H_

#include <hip/hip_runtime.h>

#include "mrp_pairhmm.h"
#include "mrp_pairhmm_dev.h" /* St, phm_log_add, phm_cell, phm_dot */
#include "mrp_wave.h"        /* lds_barrier */

#pragma clang fp contract(off)

namespace {

/* symbol i of a string; everything beyond the four bases reads the N row of the emissions (stateMachine.c:363-383) */
static __device__ __forceinline__ int phm_sym(const uint8_t *s, int i) {
    const int c = s[i];
    return c > 4 ? 4 : c;
}

/* ---- the match emission of a cell: a policy the pair's context carries.  match(M, cx, cy, xi, yi): the symbols cx, cy (0..4) that
 * stand at positions xi, yi of the two strings, -1 for the symbol before the first.  Args: what a kernel is handed for the policy ---- */
struct PhmNucleotide { /* getNucleotideMatchProb, stateMachine.c:378-383: the model's table */
    struct Args {};
    static __device__ __forceinline__ PhmNucleotide of(const Args &, int, int64_t, int64_t) { return PhmNucleotide{}; }
    __device__ __forceinline__ double match(const PhmModelDev *M, int cx, int cy, int, int) const { return M->em[cx * 5 + cy]; }
};
/* getRleNucleotideMatchProb, stateMachine.c:733-738: the same + 2.3025 * repeatSubMatrix_getLogProb(x's base, strand, observed = y's
 * count, underlying = x's count), the product taken from the host's table (PhmRepeatDev).  The symbol before the first has count 0
 * (pairwiseAligner.c:535-545).  The host has checked every count against the R of its pair's model, so the index stays inside the table;
 * the table is read through the caches, never from LDS. */
struct PhmRunLength {
    struct Args {
        const uint8_t *counts;      /* parallel to the symbol pool */
        const PhmRepeatDev *models; /* one per model */
    };
    const uint8_t *rx, *ry;
    const double *rep;
    int R;
    static __device__ __forceinline__ PhmRunLength of(const Args &a, int model, int64_t x_off, int64_t y_off) {
        const PhmRepeatDev m = a.models[model];
        return PhmRunLength{a.counts + x_off, a.counts + y_off, m.rep, m.R};
    }
    __device__ __forceinline__ double match(const PhmModelDev *M, int cx, int cy, int xi, int yi) const {
        const int u = xi >= 0 ? rx[xi] : 0, o = yi >= 0 ? ry[yi] : 0;
        return M->em[cx * 5 + cy] + rep[(cx * R + u) * R + o];
    }
};

/* what every cell of a pair reads: the pair's model, the model's transitions in registers, the two strings, the match emission */
template <class Em>
struct PhmPairCtxT {
    const PhmModelDev *M;
    double t[9];
    const uint8_t *sx, *sy;
    Em em;
};
using PhmPairCtx = PhmPairCtxT<PhmNucleotide>;
template <class Em = PhmNucleotide>
static __device__ __forceinline__ PhmPairCtxT<Em> phm_pair_ctx(const PhmModelDev *models, int model, const uint8_t *pool, int64_t x_off, int64_t y_off,
                                                               const typename Em::Args &ea = {}) {
    PhmPairCtxT<Em> c{models + model, {}, pool + x_off, pool + y_off, Em::of(ea, model, x_off, y_off)};
#pragma unroll
    for (int i = 0; i < 9; i++) c.t[i] = c.M->t[i];
    return c;
}

/* ---- where a diagonal's cells lie; at(buf, W, k): buffer k of three buffers of W cells each behind buf ---- */
struct PhmInterleaved { /* LDS: the three states of cell i side by side, from element `first` of the kernel's dynamic LDS on */
    double *lds;
    int first;
    static __device__ __forceinline__ PhmInterleaved at(double *buf, int W, int k) { return PhmInterleaved{buf, 3 * W * k}; }
    __device__ __forceinline__ St load(int i) const {
        const double *c = lds + first + 3 * i;
        return St{c[0], c[1], c[2]};
    }
    __device__ __forceinline__ void store(int i, const St &s) const {
        double *c = lds + first + 3 * i;
        c[0] = s.m;
        c[1] = s.x;
        c[2] = s.y;
    }
};
/* device memory, an array per state so that a wave's loads and stores are consecutive 8-byte accesses: cell i is element first + i of
 * each.  The kept workspace, ws_m / ws_x / ws_y [cell_first[diag0 + d] + i]; `first` stays an index because three pointers per diagonal
 * carried from diagonal to diagonal cost the forward kernels an occupancy step.  D: double, or const double where a kernel only reads */
template <class D>
struct PhmPlanarT {
    D *m, *x, *y;
    int64_t first;
    __device__ __forceinline__ St load(int i) const {
        const int64_t c = first + i; /* one index for the three: stated per array, the compiler folds `first` into three pointers */
        return St{m[c], x[c], y[c]};
    }
    __device__ __forceinline__ void store(int i, const St &s) const {
        const int64_t c = first + i;
        m[c] = s.m;
        x[c] = s.x;
        y[c] = s.y;
    }
};
using PhmPlanar = PhmPlanarT<double>;
struct PhmSlice { /* device memory, [state][W]: the planar layout with one pointer, as a buffer of a workgroup's slice has it */
    double *p;
    int W;
    static __device__ __forceinline__ PhmSlice at(double *buf, int W, int k) { return PhmSlice{buf + 3 * (size_t) W * k, W}; }
    __device__ __forceinline__ St load(int i) const { return St{p[i], p[W + i], p[2 * W + i]}; }
    __device__ __forceinline__ void store(int i, const St &s) const {
        p[i] = s.m;
        p[W + i] = s.x;
        p[2 * W + i] = s.y;
    }
};

/* ---- the (l, r) of a diagonal in x - y ---- */
struct PhmBandLimits { /* the host's band, from the pair's diagonal 0 */
    const int32_t *bnd;
    __device__ __forceinline__ void operator()(int d, int &l, int &r) const {
        l = bnd[2 * d];
        r = bnd[2 * d + 1];
    }
};
struct PhmBandOrMatrixLimits { /* band_off < 0: no anchors, the band is the whole matrix */
    const int32_t *band;
    int64_t band_off;
    int lx, ly;
    __device__ __forceinline__ void operator()(int d, int &l, int &r) const {
        if (band_off >= 0) {
            l = band[2 * (band_off + d)];
            r = band[2 * (band_off + d) + 1];
        } else {
            const int xlo = d - ly > 0 ? d - ly : 0, xhi = d < lx ? d : lx;
            l = 2 * xlo - d;
            r = 2 * xhi - d;
        }
    }
};

/* ---- who strides over a diagonal: T threads, and the barrier between two diagonals.  LDS_ONLY: a workgroup of one wave that hands its
 * diagonals on in LDS and reads nothing else it stored, so the barrier orders LDS traffic only ---- */
template <int T, bool LDS_ONLY>
struct PhmTeam {
    static constexpr int size = T;
    static __device__ __forceinline__ void barrier() { LDS_ONLY ? lds_barrier() : __syncthreads(); }
};

/* ---- where the diagonals being written (cur), d - 1 (d1; limits l1, r1) and d - 2 (d2) are ---- */
struct PhmKeptWs { /* the kept workspace of the posterior kernels; first: cell_first from the pair's diagonal 0 */
    double *m, *x, *y;
    const int64_t *first;
    __device__ __forceinline__ PhmPlanar diagonal(int d) const { return PhmPlanar{m, x, y, first[d]}; }
};
enum PhmKeep { PHM_KEEP_NONE, PHM_KEEP_ALSO, PHM_KEEP_ONLY };
/* three buffers that rotate (NONE); the same with every cell stored into the kept workspace as well (ALSO); the kept workspace alone,
 * where every cell is stored anyway, so that d - 1 and d - 2 are read back from it (ONLY; V is PhmPlanar) */
template <class V, PhmKeep KEEP>
struct PhmDiagonals {
    V cur, d1, d2;
    PhmKeptWs ws;
    PhmPlanar kept;
    int l1, r1;
    __device__ __forceinline__ void begin(int d) {
        if constexpr (KEEP == PHM_KEEP_ALSO) kept = ws.diagonal(d);
        if constexpr (KEEP == PHM_KEEP_ONLY) cur = ws.diagonal(d);
    }
    __device__ __forceinline__ void store(int i, const St &c) const {
        cur.store(i, c);
        if constexpr (KEEP == PHM_KEEP_ALSO) kept.store(i, c);
    }
    __device__ __forceinline__ void advance(int l, int r) {
        const V tmp = d2;
        d2 = d1; d1 = cur; cur = tmp;
        l1 = l; r1 = r;
    }
};

/* The cell x - y = xmy of diagonal d from its neighbours on d - 1 (limits l1, r1) and d - 2 (l2, r2): stateMachine3_cellCalculate
 * (impl/stateMachine.c:562-586) as diagonalCalculation applies it (pairwiseAligner.c:547-570; the symbol before the first is N,
 * :535-545).  A neighbour outside the band contributes what one holding LOG_ZERO contributes. */
template <class V, class Ctx>
static __device__ __forceinline__ St phm_forward_cell(int d, int xmy, int l1, int r1, int l2, int r2, const V &prev1, const V &prev2,
                                                      const Ctx &c) {
    const PhmModelDev *M = c.M;
    const double *t = c.t;
    const int x = (d + xmy) >> 1, y = (d - xmy) >> 1;
    St lower{PHM_NEG, PHM_NEG, PHM_NEG}, middle = lower, upper = lower;
    if (xmy - 1 >= l1 && xmy - 1 <= r1) lower = prev1.load((xmy - 1 - l1) >> 1);
    if (xmy + 1 >= l1 && xmy + 1 <= r1) upper = prev1.load((xmy + 1 - l1) >> 1);
    if (xmy >= l2 && xmy <= r2) middle = prev2.load((xmy - l2) >> 1);
    int cx = 4, cy = 4;
    if (x > 0) cx = phm_sym(c.sx, x - 1);
    if (y > 0) cy = phm_sym(c.sy, y - 1);
    const double eY = M->ey[cy];
    const PhmRowT ty{eY + t[4], eY + t[6], eY + t[8]};
    return phm_cell(lower, middle, upper, t, M->ex[cx], c.em.match(M, cx, cy, x - 1, y - 1), ty);
}

/* The forward diagonals 0 .. n of a pair (pairwiseAligner.c:849-903 without its total): the team strides over a diagonal's cells, a
 * cell's value does not depend on which thread computes it, and one barrier separates a diagonal from the next.  A team reads only
 * what it wrote itself.  Diagonal n is left in s.d1, its limits in s.l1, s.r1. */
template <class Team, class Storage, class Limits, class Ctx>
static __device__ __forceinline__ void phm_forward_walk(int n, Storage &s, const Limits &limits, const Ctx &c) {
    const int tid = threadIdx.x;
    int l, r, l2 = 1, r2 = 0; /* the limits of the diagonal being written and of d - 2 */
    limits(0, l, r);
    s.begin(0);
    for (int i = tid; i <= (r - l) / 2; i += Team::size) s.store(i, St{c.M->start[0], c.M->start[1], c.M->start[2]});
    Team::barrier();
    s.advance(l, r);
    for (int d = 1; d <= n; d++) {
        limits(d, l, r);
        const int width = (r - l) / 2 + 1;
        s.begin(d);
        for (int i = tid; i < width; i += Team::size) s.store(i, phm_forward_cell(d, l + 2 * i, s.l1, s.r1, l2, r2, s.d1, s.d2, c));
        Team::barrier();
        l2 = s.l1; r2 = s.r1;
        s.advance(l, r);
    }
}

/* diagonalCalculationTotalProbability on the last diagonal (pairwiseAligner.c:578-596, no diagonal beyond it): dpDiagonal_dotProduct,
 * serially in index order by the one thread that calls it -- phm_log_add is not associative */
template <class V>
static __device__ __forceinline__ double phm_last_diagonal_total(const V &last, int last_cell, const PhmModelDev *M) {
    const double e_end[3] = {M->end[0], M->end[1], M->end[2]};
    double tot = PHM_NEG;
    for (int i = 0; i <= last_cell; i++) tot = phm_log_add(tot, phm_dot(last.load(i), e_end));
    return tot;
}

/* ---- the tracebacks of the posterior half (pairwiseAligner.c:752-829) ---- */

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

/* the end state probabilities a traceback starts from, ragged only at the end of the matrix (:754-756, stateMachine.c:532-560) */
static __device__ __forceinline__ void pst_end_states(const double *t, bool at_end, int ragged_right, double *e_end) {
    if (at_end && ragged_right) {
        e_end[0] = (t[3] + t[4]) / 2.0;
        e_end[1] = t[5];
        e_end[2] = t[6];
    } else {
        e_end[0] = t[0];
        e_end[1] = t[1];
        e_end[2] = t[2];
    }
}

/* What a traceback knows before its first diagonal */
template <class Em>
struct PstTbStartT {
    PhmPairCtxT<Em> c;
    int n, slot;          /* the pair's last diagonal; where its total goes */
    const int32_t *bnd;   /* the pair's band from its diagonal 0 */
    const int64_t *first; /* and its cell_first */
    double e_end[3];
};
template <class Em = PhmNucleotide>
static __device__ __forceinline__ PstTbStartT<Em> pst_tb_start(const PstTb &tb, const PstPair *pairs, const PhmModelDev *models, const uint8_t *pool,
                                                               const int32_t *band, const int64_t *cell_first, int ragged_right,
                                                               const typename Em::Args &ea = {}) {
    const PstPair p = pairs[tb.pair];
    PstTbStartT<Em> s{phm_pair_ctx<Em>(models, p.model, pool, p.x_off, p.y_off, ea), p.lx + p.ly, p.slot, band + 2 * p.diag0, cell_first + p.diag0, {}};
    pst_end_states(s.c.t, tb.d == s.n, ragged_right, s.e_end);
    return s;
}

/* The backward cell x - y = z of diagonal dd, gathered from its successors on dd + 1 (b1; limits l1, r1) and dd + 2 (b2; l2, r2).
 *
 * The reference's diagonalCalculationBackward (:572-576 with cell_calculateBackward, :322-331) at diagonal d2 lets every cell of d2,
 * ascending in x - y, push into its lower and upper neighbour on d2 - 1 and into its middle one on d2 - 2.  Seen from the cell (dd, z)
 * that receives, in the order of arrival: the match transition of (dd + 2, z), pushed while dd + 2 was walked; then, while dd + 1 is
 * walked, the gap-y transition of (dd + 1, z - 1), whose `upper` this cell is; then the gap-x transition of (dd + 1, z + 1), whose
 * `lower` it is.  A state of the receiving cell gets one term from each, b_successor[to] + (eP + tP) with the successor's symbols; a
 * successor outside the band or beyond the traceback's first diagonal gives none. */
template <class V, class Ctx>
static __device__ __forceinline__ St pst_backward_cell(int dd, int z, int l1, int r1, int l2, int r2, const V &b1, const V &b2,
                                                       const Ctx &c) {
    const PhmModelDev *M = c.M;
    const double *t = c.t;
    const int x = (dd + z) >> 1, y = (dd - z) >> 1;
    St b{PHM_NEG, PHM_NEG, PHM_NEG};
    if (z >= l2 && z <= r2) { /* (x + 1, y + 1) */
        const double sm = b2.load((z - l2) >> 1).m;
        const double eM = c.em.match(M, phm_sym(c.sx, x), phm_sym(c.sy, y), x, y);
        b.m = phm_log_add(b.m, sm + (eM + t[0]));
        b.x = phm_log_add(b.x, sm + (eM + t[1]));
        b.y = phm_log_add(b.y, sm + (eM + t[2]));
    }
    if (z - 1 >= l1 && z - 1 <= r1) { /* (x, y + 1) */
        const double s_y = b1.load((z - 1 - l1) >> 1).y;
        const double eY = M->ey[phm_sym(c.sy, y)];
        b.m = phm_log_add(b.m, s_y + (eY + t[4]));
        b.y = phm_log_add(b.y, s_y + (eY + t[6]));
        b.x = phm_log_add(b.x, s_y + (eY + t[8]));
    }
    if (z + 1 >= l1 && z + 1 <= r1) { /* (x + 1, y) */
        const double s_x = b1.load((z + 1 - l1) >> 1).x;
        const double eX = M->ex[phm_sym(c.sx, x)];
        b.m = phm_log_add(b.m, s_x + (eX + t[3]));
        b.x = phm_log_add(b.x, s_x + (eX + t[5]));
        b.y = phm_log_add(b.y, s_x + (eX + t[7]));
    }
    return b;
}

/* diagonalCalculationTotalProbability (:578-596), a cell's term of its first dot product: forward and backward cell of diagonal dd */
static __device__ __forceinline__ double pst_total_term_here(const St &f, const St &b) {
    const double bb[3] = {b.m, b.x, b.y};
    return phm_dot(f, bb);
}
/* ... and of its second: the match state of a forward step from diagonal dd - 1 (fwd; limits lm, rm) onto the cell x - y = z of
 * dd + 1, whose backward cell is b; the step's gap states stay LOG_ZERO */
template <class V, class Ctx>
static __device__ __forceinline__ double pst_total_term_next(int dd, int z, int lm, int rm, const V &fwd, const St &b,
                                                             const Ctx &c) {
    const double *t = c.t;
    const int x = (dd + 1 + z) >> 1, y = (dd + 1 - z) >> 1;
    St mid{PHM_NEG, PHM_NEG, PHM_NEG};
    if (z >= lm && z <= rm) mid = fwd.load((z - lm) >> 1);
    int cx = 4, cy = 4;
    if (x > 0) cx = phm_sym(c.sx, x - 1);
    if (y > 0) cy = phm_sym(c.sy, y - 1);
    const double eM = c.em.match(c.M, cx, cy, x - 1, y - 1);
    const St f{phm_chain(mid.m + (eM + t[0]), mid.x + (eM + t[1]), mid.y + (eM + t[2])), PHM_NEG, PHM_NEG};
    return pst_total_term_here(f, b);
}

/* diagonalCalculationPosteriorMatchProbs / ...PosteriorProbs (:610-681): the log posterior of one state of the cell (x, y) and whether
 * it is a candidate of that state's list.  A gap before the first symbol of the string it consumes is none. */
static __device__ __forceinline__ bool pst_candidate(int list, bool in, int x, int y, double f, double b, double total, double cut, double &v) {
    v = (f + b) - total;
    return in && (list == 1 || y > 0) && (list == 2 || x > 0) && v >= cut; /* list 0: match, 1: gap x, 2: gap y */
}

}  // namespace

#endif /* MRP_PAIRHMM_WALK_H_ */
