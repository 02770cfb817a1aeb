/*
 * mrp_pairhmm.hip -- read x allele alignment likelihoods: the banded pair-HMM forward probability of the reference
 * (computeForwardProbability, impl/pairwiseAligner.c:849-903) for batches of string pairs, and the alleleReadSupports
 * loop around it (impl/bubbleGraph.c:1421-1464), and the filtered-read / filtered-variant loops after the phasing
 * (:1749-2351: the supports stay on the device, a scoring kernel reduces them), the string-chunk calls built on them and, at the end
 * of the file, the composites over the extraction's result in HBM (ha_owners_kernel, ec_classes_kernel): the haplotagging of aligned
 * reads from a phased VCF (mrp_haplotag_aligned_chunks), the phasing of aligned chunks (mrp_phase_aligned_chunks; its k-mer anchors are
 * made by mrp_anchors.hip) and the same with the filtered back half (mrp_phase_aligned_chunks_with_filtered).  gfx950 only; compiled
 * with -ffp-contract=off.
 *
 * The recursion (stateMachine3_cellCalculate, impl/stateMachine.c:562-586) gives every dp cell (x, y) three states from
 * its neighbours (x-1, y), (x-1, y-1), (x, y-1); a neighbour outside the band contributes nothing, which is what a
 * neighbour holding LOG_ZERO contributes, so the kernels keep -inf where the reference keeps NULL.  Each state is a
 * chain of three logAdd (pairwiseAligner.c:279-299: cubic interpolation in fp64, float literals, no exp / log) in the
 * reference's order.  Two mappings:
 *
 *   phm_lane_kernel   a pair per LANE, for pairs whose x string has at most 100 symbols and no anchors (their band is
 *                     the whole matrix): the lane walks its matrix row by row, the previous row lives in LDS as
 *                     row[x][state][lane] (conflict-free), the column x = 0 in registers.  All 64 lanes do useful
 *                     work in every step when the pairs of a wave have similar shapes (the host sorts them), which
 *                     is the case that matters: margin phase aligns ~25-symbol alleles to ~25-symbol read substrings,
 *                     10^5 pairs per 1 Mb chunk.  LDS per wave = 1 536 B x (longest x string of the launch class):
 *                     25 symbols -> 4 waves per CU, one per SIMD.
 *   phm_wave_kernel   a pair per WAVE for everything else (long strings, anchored bands): x+y diagonal by diagonal, a
 *                     lane per cell of the diagonal, the last two diagonals in LDS.
 *
 * Bound: fp64 VALU issue (six logAdd per cell); the kernels move ~0.1 B per flop.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_internal.h"
#include "rphmm_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int PHM_WAVE = 64;
constexpr int PHM_LANE_MAX_X = 100;    /* 100 * 1 600 B = 156 KB of the 160 KB, the rest holds the tables */
constexpr int PHM_LDS_BYTES = 160 * 1024;
#define PHM_ROWS 2 /* rows a lane of the pair-per-lane kernel advances together (measured: 1 -> 2.49 ms, 2 -> 2.11, 3 -> 2.75, 4 -> 2.61, 6 -> 3.23 for 4.8e5 pairs) */
constexpr int PHM_LANE_BYTES_PER_X = 3 * 64 * 8 + 64; /* LDS per wave and x position: three states per lane + the lane's symbol */
constexpr int PHM_ETAB = 25 * 6;       /* doubles per model in the emission + transition table */
constexpr int PHM_WAVE_MAX_WIDTH = 2048; /* 3 diagonals * 2 048 cells * 3 states * 8 B = 144 KB */

struct PhmModelDev {
    double t[9];     /* order of mrp_pair_hmm */
    double em[25];   /* [cx * 5 + cy], N rows / columns hold log(0.25^2) as written in stateMachine.c:380 */
    double ex[5], ey[5];
    double start[3]; /* stateMachine3_startStateProb / raggedStartStateProb */
    double end[3];   /* stateMachine3_endStateProb / raggedEndStateProb */
};

struct PhmPair {
    int64_t x_off, y_off;
    int64_t band_off; /* first diagonal in the band array, -1: whole matrix */
    int32_t lx, ly, model, out;
};

struct PhmLanePair { /* pair-per-lane kernel: no band */
    int64_t x_off, y_off;
    int32_t lx, ly, model, out;
};

struct St {
    double m, x, y;
};

#define PHM_NEG (-__builtin_inf())

/* lookup(), pairwiseAligner.c:282-293: the float literals are rounded to float first, as the C compiler does */
static __device__ __forceinline__ double phm_lookup(double x) {
    const bool a = x <= 1.0, b = x <= 2.5, c = x <= 4.5;
    const double c3 = a ? (double) -0.009350833524763f : b ? (double) -0.014532321752540f : c ? (double) -0.004605031767994f : (double) -0.000458661602210f;
    const double c2 = a ? (double) 0.130659527668286f : b ? (double) 0.139942324101744f : c ? (double) 0.063427417320019f : (double) 0.009695946122598f;
    const double c1 = a ? (double) 0.498799810682272f : b ? (double) 0.495635523139337f : c ? (double) 0.695956496475118f : (double) 0.930734667215156f;
    const double c0 = a ? (double) 0.693203116424741f : b ? (double) 0.692140569840976f : c ? (double) 0.514272634594009f : (double) 0.168037164329057f;
    return ((c3 * x + c2) * x + c1) * x + c0;
}
/* logAdd(), pairwiseAligner.c:295-299 */
static __device__ __forceinline__ double phm_log_add(double x, double y) {
    const bool lt = x < y;
    const double hi = lt ? y : x, lo = lt ? x : y;
    const double d = hi - lo; /* NaN for two LOG_ZEROs: not used, lo == LOG_ZERO decides first */
    return (lo == PHM_NEG || d >= 7.5) ? hi : phm_lookup(d) + lo;
}
/* The same two functions with the coefficients of the interval read from LDS (coef[interval][c3, c2, c1, c0]) instead
 * of selected with 24 v_cndmask: the pair-per-lane kernel is bound by VALU issue, its LDS pipe is mostly idle */
__device__ const float PHM_COEF[16] = {-0.009350833524763f, 0.130659527668286f, 0.498799810682272f, 0.693203116424741f,
                                       -0.014532321752540f, 0.139942324101744f, 0.495635523139337f, 0.692140569840976f,
                                       -0.004605031767994f, 0.063427417320019f, 0.695956496475118f, 0.514272634594009f,
                                       -0.000458661602210f, 0.009695946122598f, 0.930734667215156f, 0.168037164329057f};
/* (selecting the float literals' bits, 3 v_cndmask per coefficient, and widening them was 5 % slower: DESIGN.md §9) */
static __device__ __forceinline__ double phm_lookup_t(double x, const double *coef) {
    const int idx = (x > 1.0 ? 1 : 0) + (x > 2.5 ? 1 : 0) + (x > 4.5 ? 1 : 0);
    const double2 a = *reinterpret_cast<const double2 *>(coef + idx * 4);
    const double2 b = *reinterpret_cast<const double2 *>(coef + idx * 4 + 2);
    return ((a.x * x + a.y) * x + b.x) * x + b.y;
}
/* Branch-free on purpose: the interpolation is evaluated for every lane and thrown away where logAdd returns the larger
 * operand (d = inf or NaN then selects a valid table row and produces a value nobody reads).  With the conditional
 * written around the interpolation the compiler emits one basic block per logAdd, each waiting for its own LDS read, and
 * the single wave of a SIMD sits idle for the latency six times per cell; as straight-line code the three state chains
 * of a cell interleave. */
static __device__ __forceinline__ double phm_log_add_t(double x, double y, const double *coef) {
    /* the larger and the smaller operand (for x == y the reference takes hi = x, lo = y: the same two numbers) */
    const double hi = __builtin_fmax(x, y), lo = __builtin_fmin(x, y);
    const double d = hi - lo; /* inf if lo is LOG_ZERO, NaN if both are */
    const double v = phm_lookup_t(d, coef) + lo;
    return !(d < 7.5) ? hi : v; /* lo == LOG_ZERO || d >= 7.5 */
}
/* HAS_SWITCH = false: every model has TRANSITION_GAP_SWITCH_TO_X / _Y = log(0) (the shipped margin parameters), the
 * third term of the gap chains is LOG_ZERO and logAdd(a, LOG_ZERO) == a */
template <bool THIRD>
static __device__ __forceinline__ double phm_chain_t(double a, double b, double c, const double *coef) {
    const double ab = phm_log_add_t(a, b, coef);
    return THIRD ? phm_log_add_t(ab, c, coef) : ab;
}

/* toCells[to] = logAdd(toCells[to], from + (eP + tP)) three times, starting from LOG_ZERO (logAdd(LOG_ZERO, a) == a) */
static __device__ __forceinline__ double phm_chain(double a, double b, double c) { return phm_log_add(phm_log_add(a, b), c); }

struct PhmRowT { /* eP + tP of the gap-y transitions of a row (y fixed) */
    double open, extend, sw;
};
static __device__ __forceinline__ St phm_cell(const St &lower, const St &middle, const St &upper, const double *t, double eX, double eM,
                                              const PhmRowT &ty) {
    St cur;
    cur.x = phm_chain(lower.m + (eX + t[3]), lower.x + (eX + t[5]), lower.y + (eX + t[7]));
    cur.m = phm_chain(middle.m + (eM + t[0]), middle.x + (eM + t[1]), middle.y + (eM + t[2]));
    cur.y = phm_chain(upper.m + ty.open, upper.y + ty.extend, upper.x + ty.sw);
    return cur;
}
/* cell_dotProduct, pairwiseAligner.c:333-339 */
static __device__ __forceinline__ double phm_dot(const St &f, const double *e) {
    double tot = f.m + e[0];
    tot = phm_log_add(tot, f.x + e[1]);
    return phm_log_add(tot, f.y + e[2]);
}
static __device__ __forceinline__ int phm_wave_max(int v) {
    for (int o = 32; o >= 1; o >>= 1) {
        const int w = __shfl_xor(v, o, PHM_WAVE);
        v = w > v ? w : v;
    }
    return v;
}

/* LDS: coef[16] | etab[n_models][cx][cy][6] = eX + {open, extend, switch to x}, eM + {continue, from x, from y} |
 * rows[wave][x - 1][state][lane].  The waves of a workgroup share the tables and nothing else.
 *
 * A lane walks its matrix R rows at a time, row r one column behind row r - 1 (x_r = k - r in step k), so the R cells
 * of a step depend only on cells of earlier steps: left = the row's own cell of step k - 1, up / diagonal = the cells
 * of the row above from steps k - 1 / k - 2, all in registers.  Only the first row of a pass reads the LDS row (the last
 * row of the previous pass) and only the last row writes it.  With one wave per SIMD this is what hides the latency of
 * the dependent fp64 chains and of the table reads: R * 3 independent chains per step instead of 3.
 * Cells beyond a lane's own strings are computed and ignored: nothing flows from larger x or y to smaller. */
template <int R, bool HAS_SWITCH>
__global__ void __launch_bounds__(256) phm_lane_kernel(const PhmLanePair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                       const PhmModelDev *__restrict__ models, int n_models, int cap, double *__restrict__ out) {
    extern __shared__ double phm_lds[];
    double *coef = phm_lds;
    double *etab = phm_lds + 16;
    const int lane = threadIdx.x & (PHM_WAVE - 1), wave = threadIdx.x / PHM_WAVE, n_waves = blockDim.x / PHM_WAVE;
    uint8_t *wave_base = reinterpret_cast<uint8_t *>(etab + (size_t) n_models * PHM_ETAB) + (size_t) wave * cap * PHM_LANE_BYTES_PER_X;
    double *row = reinterpret_cast<double *>(wave_base) + lane;          /* [x - 1][state][lane] */
    uint8_t *symx = wave_base + (size_t) cap * 3 * PHM_WAVE * sizeof(double) + lane; /* [x - 1][lane]: the lane's x string */
    if (threadIdx.x < 16) coef[threadIdx.x] = (double) PHM_COEF[threadIdx.x];
    for (int i = threadIdx.x; i < n_models * 25; i += blockDim.x) {
        const PhmModelDev *__restrict__ Mi = models + i / 25;
        const int c = i % 25;
        const double eX = Mi->ex[c / 5], eM = Mi->em[c];
        double *e = etab + (size_t) i * 6;
        e[0] = eX + Mi->t[3];
        e[1] = eX + Mi->t[5];
        e[2] = eX + Mi->t[7];
        e[3] = eM + Mi->t[0];
        e[4] = eM + Mi->t[1];
        e[5] = eM + Mi->t[2];
    }
    __syncthreads();
    const int64_t pi = ((int64_t) blockIdx.x * n_waves + wave) * PHM_WAVE + lane;
    const bool have = pi < n_pairs;
    PhmLanePair p;
    if (have) p = pairs[pi];
    else { p.x_off = 0; p.y_off = 0; p.lx = -1; p.ly = -1; p.model = 0; p.out = 0; }
    const int lx = p.lx, ly = p.ly;
    const int mx = phm_wave_max(lx), my = phm_wave_max(ly);
    const int mx1 = mx > 1 ? mx : 1;
    const PhmModelDev *__restrict__ M = models + p.model;
    const double t_open_y = M->t[4], t_extend_y = M->t[6], t_switch_y = M->t[8];
    const uint8_t *__restrict__ sx = pool + p.x_off;
    const uint8_t *__restrict__ sy = pool + p.y_off;
    /* no global loads inside the step loop (the compiler waits for each one on the spot): the x string goes to LDS */
    for (int x = 1; x <= mx1; x++) {
        int c = 4;
        if (x <= lx) { c = sx[x - 1]; c = c > 4 ? 4 : c; }
        symx[(x - 1) * PHM_WAVE] = (uint8_t) c;
#pragma unroll
        for (int s = 0; s < 3; s++) row[((x - 1) * 3 + s) * PHM_WAVE] = PHM_NEG;
    }
    const St neg{PHM_NEG, PHM_NEG, PHM_NEG};
    St b_prev = neg; /* cell (0, y0 - 1) */
    St fin = neg;    /* cell (lx, ly) */
    const double *__restrict__ etab_m = etab + (size_t) p.model * PHM_ETAB;
    int cy_next[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        cy_next[r] = 4;
        if (r >= 1 && r <= ly) { cy_next[r] = sy[r - 1]; cy_next[r] = cy_next[r] > 4 ? 4 : cy_next[r]; }
    }
    for (int y0 = 0; y0 <= my; y0 += R) {
        const double *etab_r[R];
        double ty_open[R], ty_extend[R], ty_switch[R];
        St b0[R]; /* cell (0, y0 + r): only the gap-y state can be reached */
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int y = y0 + r;
            const int cy = cy_next[r];
            /* the y symbols of the next pass are requested now and waited for after the step loop */
            cy_next[r] = 4;
            if (y + R <= ly) { cy_next[r] = sy[y + R - 1]; cy_next[r] = cy_next[r] > 4 ? 4 : cy_next[r]; }
            const double eY = M->ey[cy];
            ty_open[r] = eY + t_open_y;
            ty_extend[r] = eY + t_extend_y;
            ty_switch[r] = eY + t_switch_y;
            etab_r[r] = etab_m + cy * 6;
            const St above = r == 0 ? b_prev : b0[r > 0 ? r - 1 : 0];
            if (y == 0) b0[r] = St{M->start[0], M->start[1], M->start[2]};
            else b0[r] = St{PHM_NEG, PHM_NEG, phm_chain_t<HAS_SWITCH>(above.m + ty_open[r], above.y + ty_extend[r], above.x + ty_switch[r], coef)};
            if (lx == 0 && y == ly) fin = b0[r];
        }
        St c1[R], c2[R]; /* the row's cells of the last two steps */
        int cxs[R];
#pragma unroll
        for (int r = 0; r < R; r++) { c1[r] = neg; c2[r] = neg; cxs[r] = 4; }
        St up0_prev = b_prev;
        for (int k = 0; k <= mx + R - 1; k++) {
            /* one basic block: no branch between the R cells, so that their chains interleave */
            const int kc = (k < 1 ? 1 : (k > mx1 ? mx1 : k)) - 1; /* steps 0 and > mx read a valid slot and ignore it */
            const double *r0 = row + (size_t) kc * 3 * PHM_WAVE;
            const St up0{r0[0], r0[PHM_WAVE], r0[2 * PHM_WAVE]};
            const int c0 = symx[kc * PHM_WAVE];
#pragma unroll
            for (int r = R - 1; r >= 1; r--) cxs[r] = cxs[r - 1];
            cxs[0] = (k >= 1 && k <= lx) ? c0 : 4;
            St nw[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int x = k - r;
                const St left = c1[r];
                const St up = r == 0 ? up0 : c1[r > 0 ? r - 1 : 0];
                const St diag = r == 0 ? up0_prev : c2[r > 0 ? r - 1 : 0];
                const double2 *__restrict__ e = reinterpret_cast<const double2 *>(etab_r[r] + cxs[r] * 30);
                const double2 e01 = e[0], e23 = e[1], e45 = e[2];
                St cur;
                cur.x = phm_chain_t<HAS_SWITCH>(left.m + e01.x, left.x + e01.y, left.y + e23.x, coef);
                cur.m = phm_chain_t<true>(diag.m + e23.y, diag.x + e45.x, diag.y + e45.y, coef);
                cur.y = phm_chain_t<HAS_SWITCH>(up.m + ty_open[r], up.y + ty_extend[r], up.x + ty_switch[r], coef);
                const bool last = x == lx && y0 + r == ly && lx >= 1;
                fin.m = last ? cur.m : fin.m;
                fin.x = last ? cur.x : fin.x;
                fin.y = last ? cur.y : fin.y;
                nw[r].m = x == 0 ? b0[r].m : cur.m;
                nw[r].x = x == 0 ? b0[r].x : cur.x;
                nw[r].y = x == 0 ? b0[r].y : cur.y;
            }
            const int xl = k - (R - 1);
            if (xl >= 1 && xl <= mx) {
                double *rl = row + (size_t) (xl - 1) * 3 * PHM_WAVE;
                rl[0] = nw[R - 1].m;
                rl[PHM_WAVE] = nw[R - 1].x;
                rl[2 * PHM_WAVE] = nw[R - 1].y;
            }
#pragma unroll
            for (int r = 0; r < R; r++) { c2[r] = c1[r]; c1[r] = nw[r]; }
            up0_prev = k == 0 ? b_prev : up0;
        }
        b_prev = b0[R - 1];
    }
    if (have) {
        const double e_end[3] = {M->end[0], M->end[1], M->end[2]};
        out[p.out] = (lx == 0 && ly == 0) ? 0.0 : phm_dot(fin, e_end); /* :860-862; the last diagonal holds one cell */
    }
}

__global__ void __launch_bounds__(PHM_WAVE) phm_wave_kernel(const PhmPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                              const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band, int W,
                                                              double *__restrict__ out) {
    extern __shared__ double phm_diag[]; /* 3 diagonals x W cells x 3 states */
    const int lane = threadIdx.x;
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PhmPair p = pairs[pi];
        const int lx = p.lx, ly = p.ly, n = lx + ly;
        if (n == 0) {
            if (lane == 0) out[p.out] = 0.0;
            continue;
        }
        const PhmModelDev *__restrict__ M = models + p.model;
        double t[9];
#pragma unroll
        for (int i = 0; i < 9; i++) t[i] = M->t[i];
        const uint8_t *__restrict__ sx = pool + p.x_off;
        const uint8_t *__restrict__ sy = pool + p.y_off;
        double *d0 = phm_diag, *d1 = phm_diag + 3 * W, *d2 = phm_diag + 6 * W; /* being written, xay - 1, xay - 2 */
        auto limits = [&](int d, int &l, int &r) {
            if (p.band_off >= 0) {
                l = band[2 * (p.band_off + d)];
                r = band[2 * (p.band_off + d) + 1];
            } else {
                const int xlo = d - ly > 0 ? d - ly : 0, xhi = d < lx ? d : lx;
                l = 2 * xlo - d;
                r = 2 * xhi - d;
            }
        };
        int l1, r1, l2 = 1, r2 = 0;
        limits(0, l1, r1);
        for (int i = lane; i <= (r1 - l1) / 2; i += PHM_WAVE) {
            d1[3 * i] = M->start[0];
            d1[3 * i + 1] = M->start[1];
            d1[3 * i + 2] = M->start[2];
        }
        __syncthreads();
        for (int d = 1; d <= n; d++) {
            int l, r;
            limits(d, l, r);
            const int width = (r - l) / 2 + 1;
            for (int i = lane; i < width; i += PHM_WAVE) {
                const int xmy = l + 2 * i;
                const int x = (d + xmy) >> 1, y = (d - xmy) >> 1;
                St lower{PHM_NEG, PHM_NEG, PHM_NEG}, middle = lower, upper = lower;
                if (xmy - 1 >= l1 && xmy - 1 <= r1) { const double *c = d1 + 3 * ((xmy - 1 - l1) >> 1); lower = St{c[0], c[1], c[2]}; }
                if (xmy + 1 >= l1 && xmy + 1 <= r1) { const double *c = d1 + 3 * ((xmy + 1 - l1) >> 1); upper = St{c[0], c[1], c[2]}; }
                if (xmy >= l2 && xmy <= r2) { const double *c = d2 + 3 * ((xmy - l2) >> 1); middle = St{c[0], c[1], c[2]}; }
                int cx = 4, cy = 4;
                if (x > 0) { cx = sx[x - 1]; cx = cx > 4 ? 4 : cx; }
                if (y > 0) { cy = sy[y - 1]; cy = cy > 4 ? 4 : cy; }
                const double eY = M->ey[cy];
                const PhmRowT ty{eY + t[4], eY + t[6], eY + t[8]};
                const St cur = phm_cell(lower, middle, upper, t, M->ex[cx], M->em[cx * 5 + cy], ty);
                d0[3 * i] = cur.m;
                d0[3 * i + 1] = cur.x;
                d0[3 * i + 2] = cur.y;
            }
            __syncthreads();
            double *tmp = d2;
            d2 = d1; d1 = d0; d0 = tmp;
            l2 = l1; r2 = r1; l1 = l; r1 = r;
        }
        /* diagonalCalculationTotalProbability on the last diagonal (:578-596, no diagonal beyond it): dpDiagonal_dotProduct */
        if (lane == 0) {
            const double e_end[3] = {M->end[0], M->end[1], M->end[2]};
            double tot = PHM_NEG;
            for (int i = 0; i <= (r1 - l1) / 2; i++) tot = phm_log_add(tot, phm_dot(St{d1[3 * i], d1[3 * i + 1], d1[3 * i + 2]}, e_end));
            out[p.out] = tot;
        }
        __syncthreads();
    }
}

/* ---------------- host ---------------- */

int fail(int code, const char *msg) { return mrp_set_error(code, "%s", msg); }

#define PHM_HIP(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

/* band_construct in closed form.  Between two consecutive anchor points P = (px, py) and N = (nx, ny) (matrix
 * coordinates; the first P is (0, 0), the last N is (lx, ly)) the reference bounds the diagonals xay in (px + py,
 * nx + ny] by xL = px - e/2, yL = ny + e/2, xU = nx + e/2, yU = py - e/2 (clamped to the matrix), :218-221; on such a
 * diagonal band_setCurrentDiagonal (:96-114) yields the smallest xmy of the right parity with xmy >= xL - yL, x >= xL,
 * y <= yL and the largest with xmy <= (xU - yU rounded UP to the parity), x <= xU, y >= yU. */
int band_closed_form(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, int64_t expansion, int32_t *L, int32_t *R,
                     int64_t *cells, int *max_width) {
    if (lx < 0 || ly < 0 || expansion < 0 || expansion % 2 != 0) return MRP_ERR_ARG;
    const int64_t e2 = expansion / 2;
    auto clamp = [](int64_t z, int64_t hi) { return z < 0 ? (int64_t) 0 : (z > hi ? hi : z); };
    L[0] = 0;
    R[0] = 0;
    int64_t total = 1;
    int mw = 1;
    int64_t px = 0, py = 0, ai = 0;
    while (px + py < lx + ly) {
        int64_t nx = lx, ny = ly;
        if (ai < n_anchors) {
            nx = anchors[2 * ai] + 1;
            ny = anchors[2 * ai + 1] + 1;
            ai++;
            if (!(nx > px && ny > py && nx <= lx && ny <= ly)) return MRP_ERR_ARG; /* asserts :206-211 */
        }
        const int64_t xL = clamp(px - e2, lx), yL = clamp(ny + e2, ly), xU = clamp(nx + e2, lx), yU = clamp(py - e2, ly);
        for (int64_t d = px + py + 1; d <= nx + ny; d++) {
            int64_t l = xL - yL, r = xU - yU;
            if ((d + l) % 2 != 0) l++;
            if ((d + r) % 2 != 0) r++;
            l = std::max(l, std::max(2 * xL - d, d - 2 * yL));
            r = std::min(r, std::min(2 * xU - d, d - 2 * yU));
            if (l > r) return MRP_ERR_ARG; /* diagonal_construct :22-27 throws */
            L[d] = (int32_t) l;
            R[d] = (int32_t) r;
            const int64_t w = (r - l) / 2 + 1;
            total += w;
            if (w > mw) mw = (int) w;
        }
        px = nx;
        py = ny;
    }
    /* the reference ignores anchors left over once (lx, ly) has been reached only if there are none: an anchor list that
     * runs past the end fails its asserts, an anchor exactly at (lx - 1, ly - 1) followed by nothing is fine */
    if (ai < n_anchors) return MRP_ERR_ARG;
    if (cells) *cells = total;
    if (max_width) *max_width = mw;
    return MRP_OK;
}

void model_to_device(const mrp_pair_hmm &m, int ragged_left, int ragged_right, PhmModelDev &d) {
    const double *t = &m.match_continue;
    for (int i = 0; i < 9; i++) d.t[i] = t[i];
    for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) d.em[x * 5 + y] = (x >= 4 || y >= 4) ? -2.772588722 : m.e_match[x * 4 + y]; /* stateMachine.c:378-383 */
    for (int s = 0; s < 5; s++) {
        d.ex[s] = s >= 4 ? -1.386294361 : m.e_gap_x[s]; /* :363-368 */
        d.ey[s] = s >= 4 ? -1.386294361 : m.e_gap_y[s];
    }
    const double ninf = -INFINITY;
    /* stateMachine.c:521-560 */
    d.start[0] = ragged_left ? ninf : 0.0;
    d.start[1] = ragged_left ? 0.0 : ninf;
    d.start[2] = ragged_left ? 0.0 : ninf;
    if (ragged_right) {
        d.end[0] = (m.gap_open_x + m.gap_open_y) / 2.0;
        d.end[1] = m.gap_extend_x;
        d.end[2] = m.gap_extend_y;
    } else {
        d.end[0] = m.match_continue;
        d.end[1] = m.match_from_gap_x;
        d.end[2] = m.match_from_gap_y;
    }
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

const int WAVE_CLASS_CAP[4] = {64, 256, 1024, PHM_WAVE_MAX_WIDTH};

/* getKmerAlignmentAnchors (pairwiseAligner.c:1563-1627) with KMER_SIZE = 20 (:1519): first occurrence of every k-mer of x
 * (getKmers :1543-1555), then over the k-mers of y found among them, in order of y, the best chain with increasing x; the
 * walk back over earlier pairs stops at the first chainable one that was a running maximum (:1592).  Appends (x, y). */
constexpr int64_t PHM_KMER = 20;
int64_t kmer_anchors(const uint8_t *sx, int64_t lx, const uint8_t *sy, int64_t ly, std::vector<int64_t> &out) {
    if (PHM_KMER > lx || PHM_KMER > ly) return 0;
    std::unordered_map<std::string_view, int64_t> first;
    first.reserve((size_t) (lx - PHM_KMER + 1) * 2);
    for (int64_t i = 0; i + PHM_KMER <= lx; i++) first.emplace(std::string_view((const char *) sx + i, (size_t) PHM_KMER), i);
    struct ChainPair { int64_t x, y, score, back; bool high; };
    std::vector<ChainPair> cp;
    int64_t max_score = 0, max_pair = -1;
    for (int64_t y = 0; y + PHM_KMER <= ly; y++) {
        auto it = first.find(std::string_view((const char *) sy + y, (size_t) PHM_KMER));
        if (it == first.end()) continue;
        ChainPair c{it->second, y, 1, -1, false};
        for (int64_t j = (int64_t) cp.size() - 1; j >= 0; j--) {
            if (cp[(size_t) j].x < c.x) {
                if (cp[(size_t) j].score + 1 > c.score) { c.score = cp[(size_t) j].score + 1; c.back = j; }
                if (cp[(size_t) j].high) break;
            }
        }
        if (c.score >= max_score) { c.high = true; max_score = c.score; max_pair = (int64_t) cp.size(); }
        cp.push_back(c);
    }
    int64_t n = 0;
    for (int64_t q = max_pair; q != -1; q = cp[(size_t) q].back) n++;
    const size_t base = out.size();
    out.resize(base + 2 * (size_t) n);
    int64_t w = n;
    for (int64_t q = max_pair; q != -1; q = cp[(size_t) q].back) {
        w--;
        out[base + 2 * (size_t) w] = cp[(size_t) q].x + PHM_KMER / 2;
        out[base + 2 * (size_t) w + 1] = cp[(size_t) q].y + PHM_KMER / 2;
    }
    return n;
}

/* A batch's pairs as phm_classify reads them, in the order of the output: pair i aligns x (an allele) to y (a read substring), both
 * in one symbol pool, with model model[i] (NULL: model 0), inside the band of the anchors (x, y) anchors[2 * anchor_off[i]] up to
 * anchors[2 * anchor_off[i + 1]] (NULL: no pair is anchored).  The arrays are a PhmPairList's or a caller's. */
struct PhmPairs {
    int64_t n;
    const int64_t *x_off;
    const int32_t *x_len;
    const int64_t *y_off;
    const int32_t *y_len;
    const uint8_t *model;
    const int64_t *anchor_off, *anchors;
};

/* The pairs of a batch as the host makes them, one after the other (add) or side by side (resize, set, counts_to_offsets) */
struct PhmPairList {
    std::vector<int64_t> x_off, y_off, anchor_off{0}, anchors;
    std::vector<int32_t> x_len, y_len;
    std::vector<uint8_t> model;
    int64_t size() const { return (int64_t) x_off.size(); }
    /* pool: the symbols, for a pair that gets k-mer anchors; NULL for an unanchored one */
    void add(int64_t xo, int32_t xl, int64_t yo, int32_t yl, int mi, const uint8_t *pool) {
        x_off.push_back(xo); x_len.push_back(xl); y_off.push_back(yo); y_len.push_back(yl); model.push_back((uint8_t) mi);
        if (pool) kmer_anchors(pool + xo, xl, pool + yo, yl, anchors);
        anchor_off.push_back((int64_t) anchors.size() / 2);
    }
    void resize(int64_t n) {
        x_off.resize((size_t) n); x_len.resize((size_t) n); y_off.resize((size_t) n); y_len.resize((size_t) n); model.resize((size_t) n);
        anchor_off.assign((size_t) n + 1, 0);
    }
    /* n_anchors: a count for now; the caller appends the anchors themselves in pair order and calls counts_to_offsets() */
    void set(int64_t i, int64_t xo, int32_t xl, int64_t yo, int32_t yl, int mi, int64_t n_anchors) {
        x_off[(size_t) i] = xo; x_len[(size_t) i] = xl; y_off[(size_t) i] = yo; y_len[(size_t) i] = yl; model[(size_t) i] = (uint8_t) mi;
        anchor_off[(size_t) i + 1] = n_anchors;
    }
    void counts_to_offsets() {
        for (size_t i = 1; i < anchor_off.size(); i++) anchor_off[i] += anchor_off[i - 1];
    }
    void append(const PhmPairList &o) {
        x_off.insert(x_off.end(), o.x_off.begin(), o.x_off.end());
        x_len.insert(x_len.end(), o.x_len.begin(), o.x_len.end());
        y_off.insert(y_off.end(), o.y_off.begin(), o.y_off.end());
        y_len.insert(y_len.end(), o.y_len.begin(), o.y_len.end());
        model.insert(model.end(), o.model.begin(), o.model.end());
        for (size_t i = 1; i < o.anchor_off.size(); i++) anchor_off.push_back(anchor_off.back() + (o.anchor_off[i] - o.anchor_off[i - 1]));
        anchors.insert(anchors.end(), o.anchors.begin(), o.anchors.end());
    }
    PhmPairs view() const {
        const bool anchored = !anchors.empty();
        return PhmPairs{size(), x_off.data(), x_len.data(), y_off.data(), y_len.data(), model.data(), anchored ? anchor_off.data() : nullptr,
                        anchored ? anchors.data() : nullptr};
    }
};

/* A pair-HMM batch in two halves.  PhmLaunch, the host half (phm_classify): the pairs sorted into launch classes, the bands, the
 * models -- the sources of the uploads, so it outlives the device half.  PhmDev, the device half (phm_enqueue): the buffers of a
 * queued launch and where the log probabilities land (d_out, indexed by pair).  Its destructor drains the stream before the buffers
 * go back to their pool, so an early return never frees what a queued copy or kernel still reads. */
struct PhmLaunch {
    int64_t cells = 0;
    int n_models = 0, table_bytes = 0; /* phm_classify: what phm_enqueue sizes the launches by */
    bool has_switch = false;
    std::vector<PhmModelDev> hm;
    HostVec<PhmLanePair> lane_pairs[4];
    HostVec<PhmPair> wave_pairs[4];
    HostVec<int32_t> band;
    HostVec<uint32_t> key; /* phm_classify's sort keys (released with the launch, not between its two halves) */
};
struct PhmDev {
    hipStream_t s = nullptr;
    DevBuf<PhmModelDev> d_models;
    DevBuf<uint8_t> d_pool;
    DevBuf<int32_t> d_band;
    DevBuf<double> d_out;
    DevBuf<PhmLanePair> d_lane[4];
    DevBuf<PhmPair> d_wave[4];
    ~PhmDev() {
        if (s) (void) hipStreamSynchronize(s);
    }
};

/* The host half of a pair-HMM batch of n_pairs > 0 pairs, no device needed: the pairs sorted into the launch classes of
 * the two kernels, the bands of the anchored ones, the models as the kernels read them.  Every error of the batch (prefixed
 * with who) is raised here, MRP_ERR_UNSUPPORTED for a diagonal beyond PHM_WAVE_MAX_WIDTH cells among them. */
int phm_classify(const char *who, const mrp_pair_hmm *models, int32_t n_models, int64_t pool_bytes, const PhmPairs &P, int64_t expansion,
                 int ragged_left, int ragged_right, PhmLaunch &L) {
    const int64_t n_pairs = P.n;
    const int64_t *x_off = P.x_off, *y_off = P.y_off, *anchor_off = P.anchor_off, *anchors = P.anchors;
    const int32_t *x_len = P.x_len, *y_len = P.y_len;
    const uint8_t *model_index = P.model;
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);

    /* classify.  The pair-per-lane kernel takes the unanchored pairs whose x string fits its LDS row next to the tables;
     * launch classes by x length (4, 3, 2, 1 waves per workgroup = per CU). */
    const int table_bytes = (16 + n_models * PHM_ETAB) * (int) sizeof(double);
    /* (-1: the tables of this many models leave no room for a row, every pair goes to the pair-per-wave kernel) */
    const int lane_max_x = PHM_LDS_BYTES - table_bytes < PHM_LANE_BYTES_PER_X ? -1 : std::min(PHM_LANE_MAX_X, (PHM_LDS_BYTES - table_bytes) / PHM_LANE_BYTES_PER_X);
    int lane_cap[4];
    for (int c = 0; c < 4; c++) lane_cap[c] = std::min(lane_max_x, (PHM_LDS_BYTES - table_bytes) / ((4 - c) * PHM_LANE_BYTES_PER_X));
    constexpr uint32_t WAVE_KEY = 0xFFFFFFFFu;
    constexpr int LY_CLIP = 4095;
    HostVec<uint32_t> &key = L.key;
    key.resize((size_t) n_pairs);
    std::atomic<int64_t> bad{-1}, cells_atomic{0};
    mrp_parallel_for((n_pairs + 16383) / 16384, 1, [&](int64_t blk) {
        int64_t c_local = 0;
        for (int64_t i = blk * 16384; i < std::min(n_pairs, (blk + 1) * 16384); i++) {
            const int64_t lx = x_len[i], ly = y_len[i];
            const int mi = model_index ? model_index[i] : 0;
            const int64_t na = anchor_off ? anchor_off[i + 1] - anchor_off[i] : 0;
            if (lx < 0 || ly < 0 || x_off[i] < 0 || y_off[i] < 0 || x_off[i] + lx > pool_bytes || y_off[i] + ly > pool_bytes || mi >= n_models || na < 0 ||
                (na > 0 && !anchors)) {
                int64_t expect = -1;
                bad.compare_exchange_strong(expect, i);
                key[(size_t) i] = WAVE_KEY;
                continue;
            }
            if (na == 0 && lx <= lane_max_x) {
                key[(size_t) i] = (uint32_t) (std::min<int64_t>(ly, LY_CLIP) << 7 | lx);
                c_local += (lx + 1) * (ly + 1);
            } else {
                key[(size_t) i] = WAVE_KEY;
            }
        }
        cells_atomic += c_local;
    });
    if (bad.load() >= 0)
        return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld lies outside the symbol pool, names a model >= %d or has bad anchor offsets", who,
                             (long long) bad.load(), n_models);
    int64_t cells = cells_atomic.load();
    /* pairs of similar shape share a wave (counting sort on (y length, x length), longest first so that the tail of a
     * launch is made of the cheap ones) */
    HostVec<PhmLanePair> *lane_pairs = L.lane_pairs;
    int64_t lane_n[4] = {0, 0, 0, 0};
    {
        std::vector<int32_t> hist((size_t) (LY_CLIP + 1) << 7, 0);
        for (int64_t i = 0; i < n_pairs; i++)
            if (key[(size_t) i] != WAVE_KEY) hist[key[(size_t) i]]++;
        int cls_of[128];
        for (int lx = 0; lx < 128; lx++) {
            int c = 0;
            while (c < 3 && lx > lane_cap[c]) c++;
            cls_of[lx] = c;
        }
        for (int64_t b = (int64_t) hist.size() - 1; b >= 0; b--) {
            const int32_t h = hist[(size_t) b];
            if (!h) continue;
            const int c = cls_of[b & 127];
            hist[(size_t) b] = (int32_t) lane_n[c];
            lane_n[c] += h;
        }
        for (int c = 0; c < 4; c++) lane_pairs[c].resize((size_t) lane_n[c]);
        for (int64_t i = 0; i < n_pairs; i++) {
            const uint32_t k = key[(size_t) i];
            if (k == WAVE_KEY) continue;
            PhmLanePair &q = lane_pairs[cls_of[k & 127]][(size_t) hist[k]++];
            q.x_off = x_off[i];
            q.y_off = y_off[i];
            q.lx = x_len[i];
            q.ly = y_len[i];
            q.model = model_index ? model_index[i] : 0;
            q.out = (int32_t) i;
        }
    }
    HostVec<PhmPair> *wave_pairs = L.wave_pairs;
    HostVec<int32_t> &band = L.band;
    std::vector<int32_t> Lb, Rb;
    for (int64_t i = 0; i < n_pairs; i++) {
        if (key[(size_t) i] != WAVE_KEY) continue;
        const int64_t lx = x_len[i], ly = y_len[i];
        const int64_t na = anchor_off ? anchor_off[i + 1] - anchor_off[i] : 0;
        PhmPair p;
        p.x_off = x_off[i];
        p.y_off = y_off[i];
        p.band_off = -1;
        p.lx = (int32_t) lx;
        p.ly = (int32_t) ly;
        p.model = model_index ? model_index[i] : 0;
        p.out = (int32_t) i;
        int width;
        if (na == 0) {
            width = (int) std::min(lx, ly) + 1;
            cells += (lx + 1) * (ly + 1);
        } else {
            if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who);
            Lb.resize((size_t) (lx + ly + 1));
            Rb.resize((size_t) (lx + ly + 1));
            int64_t c = 0;
            const int rc = band_closed_form(anchors + 2 * anchor_off[i], na, lx, ly, expansion, Lb.data(), Rb.data(), &c, &width);
            if (rc != MRP_OK) return mrp_set_error(rc, "%s: pair %lld has invalid anchors (pairwiseAligner.c:206-211)", who, (long long) i);
            cells += c;
            p.band_off = (int64_t) band.size() / 2;
            for (int64_t d = 0; d <= lx + ly; d++) { band.push_back(Lb[(size_t) d]); band.push_back(Rb[(size_t) d]); }
        }
        if (width > PHM_WAVE_MAX_WIDTH)
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d)", who, (long long) i, width, PHM_WAVE_MAX_WIDTH);
        int c = 0;
        while (width > WAVE_CLASS_CAP[c]) c++;
        wave_pairs[c].push_back(p);
    }
    for (int c = 0; c < 4; c++)
        std::sort(wave_pairs[c].begin(), wave_pairs[c].end(), [](const PhmPair &a, const PhmPair &b) {
            const int64_t ca = (int64_t) a.lx * a.ly, cb = (int64_t) b.lx * b.ly;
            return ca != cb ? ca > cb : a.out < b.out;
        });
    L.cells = cells;
    L.n_models = n_models;
    L.table_bytes = table_bytes;
    L.hm.resize((size_t) n_models);
    L.has_switch = false;
    for (int i = 0; i < n_models; i++) {
        model_to_device(models[i], ragged_left, ragged_right, L.hm[(size_t) i]);
        if (!(models[i].gap_switch_to_x == -INFINITY && models[i].gap_switch_to_y == -INFINITY)) L.has_switch = true;
    }
    return MRP_OK;
}

/* The device half: uploads what phm_classify made of n_pairs pairs over pool and queues the kernels on ctx->stream;
 * ctx->ev[0] is recorded before the first kernel.  device_pool (optional): the symbols are already on the device, written by work
 * queued on ctx->stream before this call; nothing is uploaded for them and pool is not read. */
int phm_enqueue(mrp_context *ctx, const uint8_t *pool, int64_t pool_bytes, int64_t n_pairs, const PhmLaunch &H, PhmDev &L, mrp_pairhmm_stats *stats,
                const uint8_t *device_pool = nullptr) {
    const int n_models = H.n_models, table_bytes = H.table_bytes;
    const bool has_switch = H.has_switch;
    const HostVec<PhmLanePair> *lane_pairs = H.lane_pairs;
    const HostVec<PhmPair> *wave_pairs = H.wave_pairs;
    const HostVec<int32_t> &band = H.band;
    PHM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    L.d_models.pool = L.d_pool.pool = L.d_band.pool = L.d_out.pool = &ctx->pool;
    L.s = s; /* from here on the destructor drains the stream */
    PHM_HIP(L.d_models.upload(H.hm, s));
    if (!device_pool) {
        PHM_HIP(L.d_pool.alloc((size_t) pool_bytes));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(L.d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));
        device_pool = L.d_pool.p;
    }
    PHM_HIP(L.d_band.upload(band, s));
    PHM_HIP(L.d_out.alloc((size_t) n_pairs));
    for (int c = 0; c < 4; c++) {
        L.d_lane[c].pool = L.d_wave[c].pool = &ctx->pool;
        PHM_HIP(L.d_lane[c].upload(lane_pairs[c], s));
        PHM_HIP(L.d_wave[c].upload(wave_pairs[c], s));
    }
    /* once per device (contexts of several host threads may call concurrently) */
    static PerDeviceOnce once;
    const hipError_t configured = once.run([] {
        hipError_t e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *) phm_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        return e;
    });
    PHM_HIP(configured);
    /* kernel_ms must not contain the tail of the uploads (the copy engine finishes them behind the event otherwise) */
    if (stats) PHM_HIP(hipStreamSynchronize(s));
    PHM_HIP(hipEventRecord(ctx->ev[0], s));
    for (int c = 0; c < 4; c++) {
        const int64_t n = (int64_t) lane_pairs[c].size();
        if (n == 0) continue;
        int cap = 1;
        for (const PhmLanePair &p : lane_pairs[c]) cap = std::max(cap, (int) p.lx);
        const int row_bytes = cap * PHM_LANE_BYTES_PER_X;
        const int nw = std::max(1, std::min(4, (PHM_LDS_BYTES - table_bytes) / row_bytes));
        const size_t lds = (size_t) table_bytes + (size_t) nw * row_bytes;
        const int64_t per_wg = (int64_t) nw * PHM_WAVE;
        if (has_switch)
            hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, true>), dim3((unsigned) ((n + per_wg - 1) / per_wg)), dim3((unsigned) per_wg), lds, s, L.d_lane[c].p, n, device_pool,
                               L.d_models.p, (int) n_models, cap, L.d_out.p);
        else
            hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, false>), dim3((unsigned) ((n + per_wg - 1) / per_wg)), dim3((unsigned) per_wg), lds, s, L.d_lane[c].p, n, device_pool,
                               L.d_models.p, (int) n_models, cap, L.d_out.p);
        PHM_HIP(hipGetLastError());
        if (stats) stats->pairs_lane += n;
    }
    for (int c = 0; c < 4; c++) {
        const int64_t n = (int64_t) wave_pairs[c].size();
        if (n == 0) continue;
        const int W = WAVE_CLASS_CAP[c];
        const size_t lds = (size_t) 9 * W * sizeof(double);
        hipLaunchKernelGGL(phm_wave_kernel, dim3((unsigned) std::min<int64_t>(n, 16384)), dim3(PHM_WAVE), lds, s, L.d_wave[c].p, n, device_pool,
                           L.d_models.p, L.d_band.p, W, L.d_out.p);
        PHM_HIP(hipGetLastError());
        if (stats) stats->pairs_wave += n;
    }
    return MRP_OK;
}

/* What the small entries share.  On ctx->stream: the pair-HMM kernels over P (classified first: every error of the batch is raised
 * on the host, before anything is launched) with ctx->ev[0] in front of them -- or, with no pairs, the event alone; then reduce(s, lp),
 * which uploads the entry's tables, launches its reduction over the log probabilities lp (indexed by pair; NULL with no pairs),
 * records ctx->ev[1] and queues its downloads.  Then the stream is drained, stats filled and the pool reclaimed.  reduce may keep its
 * device buffers as locals bound to ctx->pool: a block that went back to the pool is handed out again only after a reclaim().
 * The entry's tables are allocated and copied between the two events, so kernel_ms of the haplotagging entries covers those small
 * copies (and, on a cold pool, their hipMalloc) beside the kernels. */
template <class Reduce>
int phm_call(mrp_context *ctx, const char *who, const mrp_pair_hmm *models, int32_t n_models, const uint8_t *pool, int64_t pool_bytes,
             const PhmPairs &P, int64_t expansion, int ragged_left, int ragged_right, mrp_pairhmm_stats *stats, double t_begin, Reduce reduce) {
    hipStream_t s = ctx->stream;
    {
        PhmLaunch H;
        PhmDev L;
        if (P.n > 0) { /* (the host's errors first, then the device: phm_enqueue makes it current) */
            int rc = phm_classify(who, models, n_models, pool_bytes, P, expansion, ragged_left, ragged_right, H);
            if (rc == MRP_OK) rc = phm_enqueue(ctx, pool, pool_bytes, P.n, H, L, stats);
            if (rc != MRP_OK) return rc;
        } else {
            PHM_HIP(hipSetDevice(ctx->device));
            if (stats) PHM_HIP(hipStreamSynchronize(s));
            PHM_HIP(hipEventRecord(ctx->ev[0], s));
        }
        L.s = s; /* (whatever reduce has queued when it fails is drained as well) */
        const int rc = reduce(s, L.d_out.p);
        if (rc != MRP_OK) return rc;
        PHM_HIP(hipStreamSynchronize(s));
        if (stats) {
            float ms = 0.f;
            PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            stats->kernel_ms = ms;
            stats->cells = H.cells;
        }
    }
    ctx->pool.reclaim();
    if (stats) stats->total_ms = now_ms() - t_begin;
    return MRP_OK;
}

/* cachedScores of the reference's bubble loops (bubbleGraph.c:1418,1844,2221, keyed by the substring alone): for every
 * entry k of every group g (entries [first[g], first[g + 1])), owner[k] = the entry of the group whose scores k takes,
 * itself if it is scored.  Only entries with may_own[k] != 0 (NULL: all) take part; the others get owner -1 (not scored,
 * not cached).  last: among the entries of a group with equal substrings the last one owns the scores, else the first. */
void substring_owners(int64_t n_groups, const int64_t *first, const uint8_t *pool, const int64_t *off, const int32_t *len,
                      const uint8_t *may_own, bool last, std::vector<int64_t> &owner) {
    owner.assign((size_t) first[n_groups], -1);
    mrp_parallel_for(n_groups, 64, [&](int64_t g) {
        std::vector<int64_t> order;
        for (int64_t k = first[g]; k < first[g + 1]; k++)
            if (!may_own || may_own[k]) order.push_back(k);
        auto same = [&](int64_t a, int64_t c) { return len[a] == len[c] && memcmp(pool + off[a], pool + off[c], (size_t) len[a]) == 0; };
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t c) {
            if (len[a] != len[c]) return len[a] < len[c];
            const int cmp = memcmp(pool + off[a], pool + off[c], (size_t) len[a]);
            return cmp != 0 ? cmp < 0 : a < c;
        });
        for (size_t i = 0; i < order.size();) {
            size_t j = i + 1;
            while (j < order.size() && same(order[i], order[j])) j++;
            const int64_t o = last ? order[j - 1] : order[i];
            for (size_t q = i; q < j; q++) owner[(size_t) order[q]] = o;
            i = j;
        }
    });
}

/* cachedScores of bubbleGraph_partitionFilteredReadsFromPhasedVcfEntries (bubbleGraph.c:2044-2072) on the device, over the arrays the
 * extraction left in HBM (mrp_extract_device): a wave per site, a lane per entry with a lane stride (a site may hold more entries than
 * a wave has lanes).  An entry takes part if its read is MRP_READ_KEPT and, with a mask, take[read] is set (the caller's downsampling in
 * mrp_phase_aligned_chunks; NULL: every kept read); owner[p] = the LAST entry of the site that takes part and has
 * p's substring (b->reads is filled by popping, :2012-2014), p itself if none follows, -1 for an entry that takes no part.  Pass one
 * gives every entry a key (length, hash of the symbols); pass two walks the site from its end and compares symbols wherever the keys
 * agree: the hash only skips comparisons.  Every loop is bounded by the site's entry count or the substring's length; the barrier
 * between the passes is the wave's own workgroup's, and both passes of a site are run by the same wave. */
constexpr uint64_t HA_NO_KEY = ~0ull;
__global__ void __launch_bounds__(PHM_WAVE) ha_owners_kernel(const int64_t *__restrict__ first, int64_t n_sites, const int32_t *__restrict__ read,
                                                             const uint8_t *__restrict__ status, const int64_t *__restrict__ len,
                                                             const int64_t *__restrict__ off, const uint8_t *__restrict__ sym,
                                                             const uint8_t *__restrict__ take, uint64_t *key, int32_t *__restrict__ owner) {
    const int lane = threadIdx.x;
    for (int64_t v = blockIdx.x; v < n_sites; v += gridDim.x) {
        const int64_t a = first[v], b = first[v + 1];
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            uint64_t k = HA_NO_KEY;
            const int32_t r = read[p];
            if (status[r] == MRP_READ_KEPT && (!take || take[r])) {
                const uint8_t *x = sym + off[p];
                const int64_t n = len[p];
                uint32_t h = 2166136261u;
                for (int64_t i = 0; i < n; i++) h = (h ^ x[i]) * 16777619u;
                k = (uint64_t) n << 32 | h;
            }
            key[p] = k;
        }
        __syncthreads();
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint64_t k = key[p];
            int32_t o = -1;
            if (k != HA_NO_KEY) {
                o = (int32_t) p;
                const uint8_t *x = sym + off[p];
                const int64_t n = len[p];
                for (int64_t q = b - 1; q > p; q--) {
                    if (key[q] != k) continue;
                    const uint8_t *y = sym + off[q];
                    int64_t i = 0;
                    while (i < n && x[i] == y[i]) i++;
                    if (i == n) {
                        o = (int32_t) q;
                        break;
                    }
                }
            }
            owner[p] = o;
        }
    }
}

/* The classes of equal substrings of every site (what sc_filtered_task finds by sorting host symbols), over symbols that lie in HBM: a wave
 * per site, lanes striding over the site's entries, waves striding over the sites, as ha_owners_kernel.  Pass one gives EVERY entry of the
 * site a key (length, FNV-1a of the symbols) -- no mask: who may own is decided later, from indices.  Pass two gives entry p its
 * representative rep[p]: the lowest entry q <= p of the site with p's length and bytes, found by walking the site from its start and
 * comparing symbols only where the keys agree (the hash only skips comparisons; two distinct strings with one key are told apart by
 * their bytes).  Every loop is bounded by the site's entry count or a substring's length; stores are plain vector stores; the barrier
 * between the passes is the wave's own workgroup's.  LenT: int32 lengths (the public seam) or the extraction's int64 ones. */
template <typename LenT>
__global__ void __launch_bounds__(PHM_WAVE) ec_classes_kernel(const int64_t *__restrict__ first, int64_t n_sites, const LenT *__restrict__ len,
                                                              const int64_t *__restrict__ off, const uint8_t *__restrict__ sym, uint64_t *key,
                                                              int32_t *__restrict__ rep) {
    const int lane = threadIdx.x;
    for (int64_t v = blockIdx.x; v < n_sites; v += gridDim.x) {
        const int64_t a = first[v], b = first[v + 1];
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint8_t *x = sym + off[p];
            const int64_t n = len[p];
            uint32_t h = 2166136261u;
            for (int64_t i = 0; i < n; i++) h = (h ^ x[i]) * 16777619u;
            key[p] = (uint64_t) n << 32 | h;
        }
        __syncthreads();
        for (int64_t p = a + lane; p < b; p += PHM_WAVE) {
            const uint64_t k = key[p];
            const uint8_t *x = sym + off[p];
            const int64_t n = len[p];
            int32_t o = (int32_t) p;
            for (int64_t q = a; q < p; q++) {
                if (key[q] != k) continue;
                const uint8_t *y = sym + off[q];
                int64_t i = 0;
                while (i < n && x[i] == y[i]) i++;
                if (i == n) {
                    o = (int32_t) q;
                    break;
                }
            }
            rep[p] = o;
        }
    }
}

/* stMath_logAddExact (sonLib), as mrp_kernels.hip and rphmm_frame.c state it */
static __device__ __forceinline__ double ht_log_add_exact(double x, double y) {
    if (x == -__builtin_inf()) return y;
    if (y == -__builtin_inf()) return x;
    return x > y ? x + log(1.0 + exp(y - x)) : y + log(1.0 + exp(x - y));
}

struct HtEntry { /* the two log probabilities (indices into the pair-HMM output) of one read at one site */
    int32_t a, b;
    int32_t hap1; /* phasing: the read is tagged haplotype 1 (else 2) */
    int32_t live; /* the back half in the string-chunk call (fs_* kernels): the record counts; the ht_* kernels do not read it */
};

/* One entry's share of a read's two totals, bubbleGraph.c:1881-1884: the supports are floats (:1869, :1881-1882) */
static __device__ __forceinline__ void ht_partition_term(const double *__restrict__ lp, const HtEntry &x, double &t1, double &t2) {
    const double s1 = (double) (float) lp[x.a], s2 = (double) (float) lp[x.b];
    t1 += s1 - ht_log_add_exact(s1, s2);
    t2 += s2 - ht_log_add_exact(s2, s1);
}
static __device__ __forceinline__ int32_t ht_hap(double t1, double t2) { return t1 > t2 ? 1 : (t2 > t1 ? 2 : 0); }

/* One tagged entry's share of a variant's two totals, bubbleGraph.c:2274-2298 (the supports stay doubles here).  Both contributions
 * come from the same two differences, so equal supports give equal totals (an exact tie). */
static __device__ __forceinline__ void ht_phase_term(const double *__restrict__ lp, const HtEntry &x, double &c, double &t) {
    const double sa = lp[x.a], sb = lp[x.b];
    const double l = ht_log_add_exact(sa, sb);
    const double da = sa - l, db = sb - l;
    c += x.hap1 ? da : db;
    t += x.hap1 ? db : da;
}
static __device__ __forceinline__ int32_t ht_state(bool visited, double c, double t) {
    return !visited ? MRP_VARIANT_NOT_VISITED : (c > t ? MRP_VARIANT_CIS : (t > c ? MRP_VARIANT_TRANS : MRP_VARIANT_TIE));
}

/* bubbleGraph.c:1876-1925: a lane per read walks the read's sites in order */
__global__ void __launch_bounds__(256) ht_partition_kernel(const int64_t *__restrict__ first, const HtEntry *__restrict__ e,
                                                           const double *__restrict__ lp, int64_t n_reads, int32_t *__restrict__ hap,
                                                           double *__restrict__ h1, double *__restrict__ h2) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    double t1 = 0.0, t2 = 0.0;
    for (int64_t i = first[r]; i < first[r + 1]; i++) ht_partition_term(lp, e[i], t1, t2);
    hap[r] = ht_hap(t1, t2);
    h1[r] = t1;
    h2[r] = t2;
}

/* bubbleGraph.c:2274-2298: a lane per variant walks its tagged entries in order */
__global__ void __launch_bounds__(256) ht_phase_kernel(const int64_t *__restrict__ first, const uint8_t *__restrict__ visited,
                                                       const HtEntry *__restrict__ e, const double *__restrict__ lp, int64_t n_variants,
                                                       int32_t *__restrict__ state, double *__restrict__ cis, double *__restrict__ trans) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_variants) return;
    double c = 0.0, t = 0.0;
    for (int64_t i = first[v]; i < first[v + 1]; i++) ht_phase_term(lp, e[i], c, t);
    state[v] = ht_state(visited[v] != 0, c, t);
    cis[v] = c;
    trans[v] = t;
}

/* the checks both haplotagging entries share: MRP_ERR_ARG for malformed sites */
int ht_check_sites(const char *who, const mrp_haptag_sites *S, int64_t n_reads, const uint8_t *read_forward_strand) {
    if (!S || n_reads < 0 || S->n_sites < 0 || S->pool_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (n_reads > 0 && !read_forward_strand) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (S->n_sites == 0) return MRP_OK;
    if (!S->allele_first || !S->allele_off || !S->allele_len || !S->compare || !S->entry_first || (S->pool_bytes > 0 && !S->pool))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (S->allele_first[0] != 0 || S->entry_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: offsets must start at 0", who);
    for (int64_t s = 0; s < S->n_sites; s++) {
        const int64_t na = S->allele_first[s + 1] - S->allele_first[s], ne = S->entry_first[s + 1] - S->entry_first[s];
        if (na < 0 || ne < 0) return mrp_set_error(MRP_ERR_ARG, "%s: offsets not ascending at site %lld", who, (long long) s);
        if (S->compare[2 * s] < 0 || S->compare[2 * s] >= na || S->compare[2 * s + 1] < 0 || S->compare[2 * s + 1] >= na)
            return mrp_set_error(MRP_ERR_ARG, "%s: site %lld compares an allele it does not have", who, (long long) s);
    }
    const int64_t n_alleles = S->allele_first[S->n_sites], n_entries = S->entry_first[S->n_sites];
    if (n_entries > 0 && (!S->entry_read || !S->entry_off || !S->entry_len)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    for (int64_t j = 0; j < n_alleles; j++)
        if (S->allele_len[j] < 0 || S->allele_off[j] < 0 || S->allele_off[j] + S->allele_len[j] > S->pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: allele %lld lies outside the pool", who, (long long) j);
    for (int64_t k = 0; k < n_entries; k++) {
        if (S->entry_len[k] < 0 || S->entry_off[k] < 0 || S->entry_off[k] + S->entry_len[k] > S->pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: read substring %lld lies outside the pool", who, (long long) k);
        if (S->entry_read[k] < 0 || S->entry_read[k] >= n_reads) return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld names read %lld of %lld", who,
                                                                                       (long long) k, (long long) S->entry_read[k], (long long) n_reads);
    }
    return MRP_OK;
}

/* the pairs of the owning entries: (allele compare[0], entry) and (allele compare[1], entry) for every owner of an active
 * site; pair_of[k] = index of the first of the two (-1 for entries that own nothing) */
struct HtPairs {
    PhmPairList list;
    std::vector<int64_t> pair_of;
};
void ht_build_pairs(const mrp_haptag_sites *S, const std::vector<uint8_t> &active, const std::vector<int64_t> &owner,
                    const uint8_t *read_forward_strand, int64_t sv_threshold, HtPairs &P) {
    P.pair_of.assign(owner.size(), -1);
    for (int64_t s = 0; s < S->n_sites; s++) {
        if (!active[(size_t) s]) continue;
        for (int64_t k = S->entry_first[s]; k < S->entry_first[s + 1]; k++) {
            if (owner[(size_t) k] != k) continue;
            P.pair_of[(size_t) k] = P.list.size();
            for (int w = 0; w < 2; w++) {
                const int64_t j = S->allele_first[s] + S->compare[2 * s + w];
                const bool anchored = S->entry_len[k] > sv_threshold || S->allele_len[j] > sv_threshold; /* bubbleGraph.c:2253-2263 */
                P.list.add(S->allele_off[j], S->allele_len[j], S->entry_off[k], S->entry_len[k], read_forward_strand[S->entry_read[k]] ? 0 : 1,
                           anchored ? S->pool : nullptr);
            }
        }
    }
}


/* ---- mrp_phase_string_chunks: profile bytes and HP tags on the device ------------------------------------------------------
 *
 * Exactness of the profile bytes.  The byte of bubbleGraph.c:2429-2435 (rphmm_frame.c mrp_profile_seqs_from_bubbles) is
 * min(255, (int64) roundf((float) (30 (total - lp)))) with lp the float support and total = logAddExact over the alleles in
 * allele order.  Everything but total is exact IEEE arithmetic on both sides (the narrowing to float, the fp64 subtraction and
 * product -- not contracted in this file --, the conversion to float, roundf, and the x86 conversion restated below).  total
 * takes one exp and one log per allele after the first: the device's (ocml) and glibc's double exp / log are both faithfully
 * rounded, so total can differ from the host's in its last bit, 2^-52 relative: about 1e-14 absolute for the values here (|total|
 * below 10^3).  That moves 30 (total - lp) by less than 1e-12, and the byte changes only if the fp64 value lies that close to a
 * point where its float rounding crosses a half integer; float spacing below 256 is at least 2^-16, so the chance is below
 * 1e-7 per byte, and the supports are the same floats on both sides.  The tests compare every byte of the chain's pool. */
static __device__ __forceinline__ int64_t sc_f32_to_i64_x86(float v) { /* (int64_t) of a float as x86-64 converts it (cvttss2si) */
    if (!(v >= -9223372036854775808.0f && v < 9223372036854775808.0f)) return INT64_MIN;
    return (int64_t) v;
}

struct ScByteItem { /* one (bubble, read substring): where its bytes go in the device pool, the first pair of its owner */
    int64_t dst;
    int32_t pair;      /* the owner's pair with allele 0 of the bubble; alleles follow */
    int32_t n_alleles;
};

/* bubbleGraph.c:2421-2435 over the supports of bubbleGraph.c:1421-1464: a lane per (bubble, substring) */
__global__ void __launch_bounds__(256) sc_profile_bytes_kernel(const ScByteItem *__restrict__ items, int64_t n_items, const double *__restrict__ lp,
                                                               uint8_t *__restrict__ pool) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const ScByteItem it = items[i];
    const double *p = lp + it.pair;
    double total = -__builtin_inf();
    for (int32_t k = 0; k < it.n_alleles; k++) total = ht_log_add_exact(total, (double) (float) p[k]); /* the float store of :1464 */
    uint8_t *dst = pool + it.dst;
    for (int32_t k = 0; k < it.n_alleles; k++) {
        const float f = (float) p[k];
        const int64_t l = sc_f32_to_i64_x86(roundf((float) (30.0 * (total - (double) f))));
        dst[k] = (uint8_t) (l > 255 ? 255 : l);
    }
}

struct ScHapItem { /* one profile sequence of one chunk */
    int64_t pool;   /* its bytes in the device pool */
    int64_t aoff;   /* its chunk's allele offsets (n_sites + 1) in the offsets table */
    int64_t hap;    /* its chunk's haplotype strings: hap1 then hap2, frag_length each */
    int32_t ref_start, length, frag_start, frag_length;
    int32_t side;   /* 1 / 2: in reads1 / only in reads2 of the fragment, 0: in neither */
    int32_t pad;
};

/* stGenomeFragment_phaseBamChunkReads (genomeFragment.c:234-276) with getLogProbOfReadGivenHaplotype (:71-89) and
 * getLogProbabilityOfBeingInPartition (:91-100), as mrp_assign_reads_to_haplotypes states them: a lane per sequence.  The
 * sums of bytes are integers, exact in fp64 in any order; one exp and one log follow (relative error ~1e-16). */
__global__ void __launch_bounds__(256) sc_assign_kernel(const ScHapItem *__restrict__ items, int64_t n_items, const int64_t *__restrict__ aoff,
                                                        const uint64_t *__restrict__ haps, const uint8_t *__restrict__ pool, int64_t min_phred,
                                                        int8_t *__restrict__ hap_out, double *__restrict__ phred_out) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const ScHapItem it = items[i];
    if (it.side == 0) { hap_out[i] = -1; phred_out[i] = 0.0; return; }
    /* :255-259: the first haplotype handed over for a hap1 read is haplotypeString2, i.e. the OTHER one */
    const uint64_t *mine = haps + it.hap + (it.side == 1 ? 0 : it.frag_length), *other = haps + it.hap + (it.side == 1 ? it.frag_length : 0);
    const int64_t *ao = aoff + it.aoff + it.ref_start;
    const uint8_t *bytes = pool + it.pool;
    int32_t lo = it.frag_start - it.ref_start, hi = it.frag_start + it.frag_length - it.ref_start;
    if (lo < 0) lo = 0;
    if (hi > it.length) hi = it.length;
    double ta = 0.0, tb = 0.0;
    for (int32_t s = lo; s < hi; s++) {
        const int64_t o = ao[s] - ao[0], A = ao[s + 1] - ao[s];
        const int64_t j = (int64_t) s + it.ref_start - it.frag_start;
        const uint64_t ho = other[j], hm = mine[j];
        if (ho < (uint64_t) A) ta -= bytes[o + (int64_t) ho]; /* (a haplotype allele is always one of the site's) */
        if (hm < (uint64_t) A) tb -= bytes[o + (int64_t) hm];
    }
    const double a = ta / 30.0, b = tb / 30.0;
    const double lp = a - ht_log_add_exact(a, b);
    const double phred = -10 * lp / 2.302585; /* :260 */
    hap_out[i] = phred < (double) min_phred ? 0 : (int8_t) it.side;
    phred_out[i] = phred;
}

/* what the host works out for one chunk beside the pair-HMM kernels: bubbleGraph_getProfileSeqs' layout (bubbleGraph.c:2356-2381)
 * and bubbleGraph_getReference's tables (:2443-2474), as rphmm_frame.c computes them */
struct ScLayout {
    std::vector<mrp_read> seqs;
    std::vector<int32_t> read_of_seq, seq_of;
    std::vector<int64_t> aoff; /* n_bubbles + 1 */
    int64_t pool_bytes = 0;
    std::vector<uint32_t> an;
    std::vector<uint16_t> sub, prior;
};

/* (uint16_t) of a float as gcc/x86-64 converts it (rphmm_frame.c) */
uint16_t sc_f32_to_u16_x86(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return 0;
    return (uint16_t) (uint32_t) (int32_t) v;
}

/* MRP_ERR_ARG for a malformed chunk; seen: scratch of n_reads entries */
int sc_check_chunk(const char *who, int64_t c, const mrp_string_chunk &S, std::vector<int64_t> &seen) {
    if (S.n_bubbles < 0 || S.n_reads < 0 || S.pool_bytes < 0 || S.n_reads >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes", who, (long long) c);
    if (S.n_reads > 0 && (!S.read_names || !S.read_forward_strand)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    for (int64_t r = 0; r < S.n_reads; r++)
        if (!S.read_names[r]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %lld has no name", who, (long long) c, (long long) r);
    if (S.n_bubbles == 0) return MRP_OK;
    if (!S.allele_first || !S.sub_first || (S.pool_bytes > 0 && !S.pool)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    if (S.allele_first[0] != 0 || S.sub_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets must start at 0", who, (long long) c);
    for (int64_t b = 0; b < S.n_bubbles; b++) {
        const int64_t na = S.allele_first[b + 1] - S.allele_first[b], ns = S.sub_first[b + 1] - S.sub_first[b];
        if (na < 1 || na > 65535 || ns < 0)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets not ascending or no allele at bubble %lld", who, (long long) c, (long long) b);
    }
    const int64_t n_alleles = S.allele_first[S.n_bubbles], n_subs = S.sub_first[S.n_bubbles];
    if (!S.allele_off || !S.allele_len || (n_subs > 0 && (!S.sub_off || !S.sub_len || !S.sub_read)))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument", who, (long long) c);
    for (int64_t j = 0; j < n_alleles; j++)
        if (S.allele_len[j] < 0 || S.allele_off[j] < 0 || S.allele_off[j] + S.allele_len[j] > S.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: allele %lld lies outside the pool", who, (long long) c, (long long) j);
    seen.assign((size_t) S.n_reads, -1);
    for (int64_t b = 0; b < S.n_bubbles; b++)
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            if (S.sub_len[k] < 0 || S.sub_off[k] < 0 || S.sub_off[k] + S.sub_len[k] > S.pool_bytes)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read substring %lld lies outside the pool", who, (long long) c, (long long) k);
            const int32_t r = S.sub_read[k];
            if (r < 0 || r >= S.n_reads)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: substring %lld names read %d of %lld", who, (long long) c, (long long) k, r, (long long) S.n_reads);
            if (seen[(size_t) r] == b) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %d appears twice in bubble %lld", who, (long long) c, r, (long long) b);
            seen[(size_t) r] = b;
        }
    return MRP_OK;
}

void sc_layout(const mrp_string_chunk &S, double het_substitution_probability, ScLayout &Lc) {
    const int64_t nb = S.n_bubbles, n_reads = S.n_reads;
    std::vector<int64_t> first((size_t) n_reads, -1), last((size_t) n_reads, -1);
    Lc.seq_of.assign((size_t) n_reads, -1);
    Lc.read_of_seq.clear();
    for (int64_t b = 0; b < nb; b++)
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            const int32_t r = S.sub_read[k];
            if (first[(size_t) r] < 0) { first[(size_t) r] = b; Lc.seq_of[(size_t) r] = (int32_t) Lc.read_of_seq.size(); Lc.read_of_seq.push_back(r); }
            last[(size_t) r] = b;
        }
    Lc.aoff.assign((size_t) nb + 1, 0);
    Lc.an.resize((size_t) nb);
    int64_t n_sub = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int64_t A = S.allele_first[b + 1] - S.allele_first[b];
        Lc.an[(size_t) b] = (uint32_t) A;
        Lc.aoff[(size_t) b + 1] = Lc.aoff[(size_t) b] + A;
        n_sub += A * A;
    }
    const int64_t n_seqs = (int64_t) Lc.read_of_seq.size();
    Lc.seqs.assign((size_t) n_seqs, mrp_read{});
    int64_t pool_bytes = 0;
    for (int64_t q = 0; q < n_seqs; q++) { /* stProfileSeq_constructEmptyProfile profileSeq.c:13-29 */
        const int32_t r = Lc.read_of_seq[(size_t) q];
        mrp_read &m = Lc.seqs[(size_t) q];
        m.name = S.read_names[r];
        m.ref_start = (int32_t) first[(size_t) r];
        m.length = (int32_t) (last[(size_t) r] - first[(size_t) r] + 1);
        m.forward_strand = S.read_forward_strand[r] ? 1 : 0;
        m.pool_offset = pool_bytes;
        pool_bytes += Lc.aoff[(size_t) last[(size_t) r] + 1] - Lc.aoff[(size_t) first[(size_t) r]];
    }
    Lc.pool_bytes = pool_bytes;
    /* bubbleGraph.c:2458-2467 */
    const uint16_t off = sc_f32_to_u16_x86(roundf((float) (-log(het_substitution_probability) * 30.0)));
    Lc.sub.assign((size_t) n_sub, 0);
    Lc.prior.assign((size_t) Lc.aoff[(size_t) nb], 0);
    int64_t o = 0;
    for (int64_t b = 0; b < nb; b++) {
        const int64_t A = Lc.an[(size_t) b];
        for (int64_t j = 0; j < A; j++)
            for (int64_t k = 0; k < A; k++) Lc.sub[(size_t) (o + j * A + k)] = j == k ? 0 : off;
        o += A * A;
    }
}

/* ---- the back half in the string-chunk call (mrp_phase_string_chunks_with_filtered) ------------------------------
 * A "site" is a primary bubble of a chunk with a rest (its entries: the bubble's primary substrings and the filtered reads') or a
 * filtered variant (its entries as listed).  The front groups a site's entries into classes of equal substrings and scores, for
 * every class and every strand that occurs in it, the pairs some outcome of the phasing could read: cbase[2 * class + reverse] is
 * the block of that (class, strand) in pidx, pidx[block + allele] (bubbles) / pidx[block + 0 / 1] (variants: gt1, gt2) the pair. */
struct FsEntry {
    int32_t cls;   /* class within the site */
    int32_t read;  /* the call's read index (primary reads of a chunk first, then its filtered reads) */
    int32_t key;   /* position in the site's listing order: the owner of a class is the max (bubbles) / min (variants) over its
                    * participating entries */
    int32_t flags; /* 1: reverse strand, 2: a filtered read */
};
struct FsSite {
    int64_t entry_first, cls_first;
    int32_t n_entries, n_classes;
    int32_t chunk, bubble; /* bubble < 0: a variant */
    int32_t n_alleles, visited; /* variants: gt1 != gt2 and entries (bubbleGraph.c:2174, :2186-2192) */
};
struct FsChunk { /* what the phasing decided for a chunk: where its haplotype strings are (hap1 then hap2, frag_length each) */
    int64_t hap;
    int32_t frag_start, frag_length;
};
constexpr int FS_TILE = 256; /* classes per pass of the LDS owner table */

/* the tag of a read where the HP kernel wrote it: read_seq = its profile sequence, -1 a primary read in no bubble, -2 a filtered read */
static __device__ __forceinline__ int fs_tag(const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags, int32_t read) {
    const int32_t q = read_seq[read];
    return q >= 0 ? (int) tags[q] : -1;
}

/* A wave per site, behind sc_assign_kernel.  Decides the site's activity and its two alleles (bubbles: the fragment's hap1 / hap2
 * allele, bubbleGraph.c:1780; variants: gt1 / gt2), each entry's participation (bubbles: filtered reads and untagged primary
 * reads; variants: tagged primary reads, :2226-2235), per class the owning entry (bubbles: the last-listed participant, :1816-1819;
 * variants: the first, :2221) and from the owner's strand the two pairs.  One record per entry, live or not. */
__global__ void __launch_bounds__(64) sc_filtered_sites_kernel(const FsSite *__restrict__ sites, const FsEntry *__restrict__ ent,
                                                               const int32_t *__restrict__ cbase, const int32_t *__restrict__ pidx,
                                                               const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags,
                                                               const FsChunk *__restrict__ chunks, const uint64_t *__restrict__ haps,
                                                               HtEntry *__restrict__ rec, uint8_t *__restrict__ used) {
    __shared__ int32_t tab[FS_TILE];
    const FsSite st = sites[blockIdx.x];
    const int lane = (int) threadIdx.x;
    const bool variant = st.bubble < 0;
    bool active = st.visited != 0;
    int32_t a1 = 0, a2 = 1;
    if (!variant) {
        const FsChunk ch = chunks[st.chunk];
        const int32_t j = st.bubble - ch.frag_start;
        active = j >= 0 && j < ch.frag_length;
        if (active) {
            const uint64_t h1 = haps[ch.hap + j], h2 = haps[ch.hap + ch.frag_length + j];
            active = h1 != h2 && h1 < (uint64_t) st.n_alleles && h2 < (uint64_t) st.n_alleles;
            a1 = (int32_t) h1;
            a2 = (int32_t) h2;
        }
    }
    const FsEntry *e = ent + st.entry_first;
    HtEntry *out = rec + st.entry_first;
    for (int32_t i = lane; i < st.n_entries; i += 64) out[i] = HtEntry{0, 0, 0, 0};
    if (!active) return; /* (the same for every lane of the block) */
    for (int32_t t0 = 0; t0 < st.n_classes; t0 += FS_TILE) {
        for (int i = lane; i < FS_TILE; i += 64) tab[i] = variant ? INT32_MAX : -1;
        __syncthreads();
        for (int32_t i = lane; i < st.n_entries; i += 64) {
            const FsEntry x = e[i];
            const int tag = fs_tag(read_seq, tags, x.read);
            const bool tagged = !(x.flags & 2) && (tag == 1 || tag == 2);
            const bool takes_part = variant ? tagged : !tagged;
            if (!takes_part || x.cls < t0 || x.cls >= t0 + FS_TILE) continue;
            const int32_t v = x.key * 2 + (x.flags & 1);
            if (variant) atomicMin(&tab[x.cls - t0], v);
            else atomicMax(&tab[x.cls - t0], v);
        }
        __syncthreads();
        for (int32_t i = lane; i < st.n_entries; i += 64) {
            const FsEntry x = e[i];
            const int tag = fs_tag(read_seq, tags, x.read);
            const bool tagged = !(x.flags & 2) && (tag == 1 || tag == 2);
            const bool takes_part = variant ? tagged : !tagged;
            if (!takes_part || x.cls < t0 || x.cls >= t0 + FS_TILE) continue;
            const int32_t owner = tab[x.cls - t0];
            const int32_t block = cbase[2 * (st.cls_first + x.cls) + (owner & 1)];
            const int32_t pa = pidx[block + a1], pb = pidx[block + a2];
            out[i] = HtEntry{pa, pb, tag == 1 ? 1 : 0, 1};
            if (used) { used[pa] = 1; used[pb] = 1; }
        }
        __syncthreads();
    }
}

/* ht_partition_kernel over a read's static candidate list (its entries at bubbles, in bubble order): records that are not live
 * are skipped.  A primary read the phasing tagged keeps its tag. */
__global__ void __launch_bounds__(256) fs_partition_kernel(const int64_t *__restrict__ first, const int32_t *__restrict__ cand,
                                                           const HtEntry *__restrict__ e, const double *__restrict__ lp,
                                                           const int32_t *__restrict__ read_seq, const int8_t *__restrict__ tags, int64_t n_reads,
                                                           int32_t *__restrict__ hap, double *__restrict__ h1, double *__restrict__ h2) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int tag = fs_tag(read_seq, tags, (int32_t) r);
    if (read_seq[r] != -2 && (tag == 1 || tag == 2)) { hap[r] = tag; h1[r] = 0.0; h2[r] = 0.0; return; }
    double t1 = 0.0, t2 = 0.0;
    for (int64_t i = first[r]; i < first[r + 1]; i++) {
        const HtEntry x = e[cand[i]];
        if (x.live) ht_partition_term(lp, x, t1, t2);
    }
    hap[r] = ht_hap(t1, t2);
    h1[r] = t1;
    h2[r] = t2;
}

/* ht_phase_kernel over a variant's entries in order, the records that are not live skipped */
__global__ void __launch_bounds__(256) fs_phase_kernel(const FsSite *__restrict__ sites, const HtEntry *__restrict__ e, const double *__restrict__ lp,
                                                       int64_t n_variants, int32_t *__restrict__ state, double *__restrict__ cis,
                                                       double *__restrict__ trans) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_variants) return;
    const FsSite st = sites[v];
    double c = 0.0, t = 0.0;
    for (int64_t i = st.entry_first; i < st.entry_first + st.n_entries; i++) {
        const HtEntry x = e[i];
        if (x.live) ht_phase_term(lp, x, c, t);
    }
    state[v] = ht_state(st.visited != 0, c, t);
    cis[v] = c;
    trans[v] = t;
}

bool sc_rest_empty(const mrp_string_chunk_rest &R) { return R.n_filtered == 0 && R.n_variants == 0; }

/* MRP_ERR_ARG for a malformed rest of chunk c (the chunk itself has passed sc_check_chunk) */
int sc_check_rest(const char *who, int64_t c, const mrp_string_chunk &S, const mrp_string_chunk_rest &R) {
    const long long cc = (long long) c;
    if (R.n_filtered < 0 || R.n_variants < 0 || R.pool_bytes < 0 || S.n_reads + R.n_filtered >= (1ll << 30))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes of the rest", who, cc);
    if ((R.n_filtered > 0 && !R.forward_strand) || (R.pool_bytes > 0 && !R.pool)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    if (R.n_filtered > 0 && S.n_bubbles > 0 && !R.fsub_first) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest (fsub_first)", who, cc);
    if (R.fsub_first && S.n_bubbles > 0) {
        if (R.fsub_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets of the rest must start at 0", who, cc);
        for (int64_t b = 0; b < S.n_bubbles; b++)
            if (R.fsub_first[b + 1] < R.fsub_first[b])
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring offsets not ascending at bubble %lld", who, cc, (long long) b);
        const int64_t n = R.fsub_first[S.n_bubbles];
        if (n > 0 && (!R.fsub_off || !R.fsub_len || !R.fsub_read)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = R.fsub_first[b]; k < R.fsub_first[b + 1]; k++) {
                if (R.fsub_len[k] < 0 || R.fsub_off[k] < 0 || R.fsub_off[k] + R.fsub_len[k] > R.pool_bytes)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring %lld lies outside the pool", who, cc, (long long) k);
                const int32_t r = R.fsub_read[k];
                if (r < 0 || r >= R.n_filtered)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered substring %lld names read %d of %lld", who, cc, (long long) k, r, (long long) R.n_filtered);
                if (k > R.fsub_first[b] && R.fsub_read[k - 1] == r)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered read %d appears twice in bubble %lld", who, cc, r, (long long) b);
                if (k > R.fsub_first[b] && R.fsub_read[k - 1] > r)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: filtered reads of bubble %lld are not in ascending order", who, cc, (long long) b);
            }
    }
    if (R.n_variants == 0) return MRP_OK;
    if (!R.valle_first || !R.ventry_first || !R.gt) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    if (R.valle_first[0] != 0 || R.ventry_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets of the rest must start at 0", who, cc);
    for (int64_t v = 0; v < R.n_variants; v++) {
        const int64_t na = R.valle_first[v + 1] - R.valle_first[v], ne = R.ventry_first[v + 1] - R.ventry_first[v];
        if (na < 0 || ne < 0 || ne >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: offsets not ascending at variant %lld", who, cc, (long long) v);
        if (R.gt[2 * v] < 0 || R.gt[2 * v] >= na || R.gt[2 * v + 1] < 0 || R.gt[2 * v + 1] >= na)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant %lld has a genotype allele it does not have", who, cc, (long long) v);
    }
    const int64_t n_alleles = R.valle_first[R.n_variants], n_entries = R.ventry_first[R.n_variants];
    if ((n_alleles > 0 && (!R.valle_off || !R.valle_len)) || (n_entries > 0 && (!R.ventry_read || !R.ventry_off || !R.ventry_len)))
        return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null argument in the rest", who, cc);
    for (int64_t j = 0; j < n_alleles; j++)
        if (R.valle_len[j] < 0 || R.valle_off[j] < 0 || R.valle_off[j] + R.valle_len[j] > R.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant allele %lld lies outside the pool", who, cc, (long long) j);
    for (int64_t k = 0; k < n_entries; k++) {
        if (R.ventry_len[k] < 0 || R.ventry_off[k] < 0 || R.ventry_off[k] + R.ventry_len[k] > R.pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant entry %lld lies outside the pool", who, cc, (long long) k);
        if (R.ventry_read[k] < 0 || R.ventry_read[k] >= S.n_reads + R.n_filtered)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant entry %lld names read %d of %lld", who, cc, (long long) k, R.ventry_read[k],
                                 (long long) (S.n_reads + R.n_filtered));
    }
    return MRP_OK;
}

}  // namespace

extern "C" {

void mrp_symbols_from_chars(const char *s, int64_t n, uint8_t *out) {
    for (int64_t i = 0; i < n; i++) {
        switch (s[i]) {
            case 'A': case 'a': out[i] = 0; break;
            case 'C': case 'c': out[i] = 1; break;
            case 'G': case 'g': out[i] = 2; break;
            case 'T': case 't': out[i] = 3; break;
            default: out[i] = 4;
        }
    }
}

void mrp_pair_hmm_reverse_complement(mrp_pair_hmm *m) {
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++) std::swap(m->e_match[i * 4 + j], m->e_match[(3 - i) * 4 + (3 - j)]);
    std::swap(m->e_match[0], m->e_match[15]);
    std::swap(m->e_match[5], m->e_match[10]);
    for (int i = 0; i < 2; i++) {
        std::swap(m->e_gap_x[i], m->e_gap_x[3 - i]);
        std::swap(m->e_gap_y[i], m->e_gap_y[3 - i]);
    }
}

int64_t mrp_kmer_alignment_anchors(const uint8_t *x, int64_t lx, const uint8_t *y, int64_t ly, int64_t *out) {
    if (!out || lx < 0 || ly < 0 || (lx > 0 && !x) || (ly > 0 && !y)) return 0;
    std::vector<int64_t> v;
    const int64_t n = kmer_anchors(x, lx, y, ly, v);
    if (n > 0) memcpy(out, v.data(), sizeof(int64_t) * 2 * (size_t) n);
    return n;
}

int mrp_band_diagonals(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, int64_t expansion, int32_t *xmy_l, int32_t *xmy_r) {
    if (!xmy_l || !xmy_r || (n_anchors > 0 && !anchors) || n_anchors < 0) return fail(MRP_ERR_ARG, "mrp_band_diagonals: null argument");
    if (lx + ly >= (1ll << 30)) return fail(MRP_ERR_ARG, "mrp_band_diagonals: strings too long");
    const int rc = band_closed_form(anchors, n_anchors, lx, ly, expansion, xmy_l, xmy_r, nullptr, nullptr);
    return rc == MRP_OK ? rc : fail(rc, "mrp_band_diagonals: invalid anchors or expansion (pairwiseAligner.c:179,206-211)");
}

int mrp_forward_probabilities(mrp_context *ctx, const mrp_pair_hmm *models, int32_t n_models, int64_t n_pairs, const uint8_t *pool,
                              int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len, const int64_t *y_off, const int32_t *y_len,
                              const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors, int64_t expansion, int ragged_left,
                              int ragged_right, double *out, mrp_pairhmm_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_forward_probabilities: no context (the pair-HMM path has no CPU fallback)");
    if (n_pairs < 0 || n_models <= 0 || !models || pool_bytes < 0) return fail(MRP_ERR_ARG, "mrp_forward_probabilities: bad sizes");
    if (n_pairs == 0) return MRP_OK;
    if (!x_off || !x_len || !y_off || !y_len || !out || (pool_bytes > 0 && !pool)) return fail(MRP_ERR_ARG, "mrp_forward_probabilities: null argument");
    const PhmPairs P{n_pairs, x_off, x_len, y_off, y_len, model_index, anchor_off, anchors};
    return phm_call(ctx, "mrp_forward_probabilities", models, n_models, pool, pool_bytes, P, expansion, ragged_left, ragged_right, stats, t_begin,
                    [&](hipStream_t s, const double *lp) {
                        PHM_HIP(hipEventRecord(ctx->ev[1], s));
                        PHM_HIP(hipMemcpyAsync(out, lp, (size_t) n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
                        return (int) MRP_OK;
                    });
}

int mrp_allele_read_supports(mrp_context *ctx, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t n_bubbles,
                             const int64_t *allele_first, const int64_t *read_first, const uint8_t *pool, int64_t pool_bytes,
                             const int64_t *allele_off, const int32_t *allele_len, const int64_t *read_off, const int32_t *read_len,
                             const uint8_t *read_forward_strand, int64_t expansion, int64_t sv_threshold, float *support,
                             mrp_pairhmm_stats *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_allele_read_supports: no context (the pair-HMM path has no CPU fallback)");
    if (n_bubbles < 0) return fail(MRP_ERR_ARG, "mrp_allele_read_supports: bad sizes");
    if (n_bubbles == 0) return MRP_OK;
    if (!forward_model || !reverse_model || !allele_first || !read_first || !allele_off || !allele_len || !read_off || !read_len ||
        !read_forward_strand || !support || (pool_bytes > 0 && !pool))
        return fail(MRP_ERR_ARG, "mrp_allele_read_supports: null argument");
    const int64_t n_reads_total = read_first[n_bubbles];
    for (int64_t k = 0; k < n_reads_total; k++)
        if (read_len[k] < 0 || read_off[k] < 0 || read_off[k] + read_len[k] > pool_bytes) return fail(MRP_ERR_ARG, "mrp_allele_read_supports: read substring outside the pool");
    /* cachedScores (bubbleGraph.c:1418,1431-1441): the first read of the bubble with a given substring owns the scores */
    std::vector<int64_t> owner;
    substring_owners(n_bubbles, read_first, pool, read_off, read_len, nullptr, false, owner);
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    PhmPairList pairs;
    std::vector<int64_t> where;
    std::vector<int64_t> support_first((size_t) n_bubbles + 1, 0);
    for (int64_t b = 0; b < n_bubbles; b++) {
        const int64_t na = allele_first[b + 1] - allele_first[b], nr = read_first[b + 1] - read_first[b];
        if (na < 0 || nr < 0) return fail(MRP_ERR_ARG, "mrp_allele_read_supports: offsets not ascending");
        support_first[(size_t) b + 1] = support_first[(size_t) b] + na * nr;
        for (int64_t k = read_first[b]; k < read_first[b + 1]; k++) {
            if (owner[(size_t) k] != k) continue;
            for (int64_t j = allele_first[b]; j < allele_first[b + 1]; j++) {
                where.push_back(support_first[(size_t) b] + (j - allele_first[b]) * nr + (k - read_first[b]));
                const bool anchored = read_len[k] > sv_threshold || allele_len[j] > sv_threshold; /* bubbleGraph.c:1448-1451 */
                if (anchored && (allele_len[j] < 0 || allele_off[j] < 0 || allele_off[j] + allele_len[j] > pool_bytes))
                    return fail(MRP_ERR_ARG, "mrp_allele_read_supports: allele outside the pool");
                pairs.add(allele_off[j], allele_len[j], read_off[k], read_len[k], read_forward_strand[k] ? 0 : 1, anchored ? pool : nullptr);
            }
        }
    }
    std::vector<double> lp((size_t) pairs.size());
    const PhmPairs P = pairs.view();
    const int rc = mrp_forward_probabilities(ctx, models, 2, P.n, pool, pool_bytes, P.x_off, P.x_len, P.y_off, P.y_len, P.model, P.anchor_off, P.anchors, expansion,
                                             0, 0, lp.data(), stats);
    if (rc != MRP_OK) return rc;
    for (size_t i = 0; i < lp.size(); i++) support[where[i]] = (float) lp[i];
    for (int64_t b = 0; b < n_bubbles; b++) {
        const int64_t na = allele_first[b + 1] - allele_first[b], nr = read_first[b + 1] - read_first[b];
        for (int64_t k = 0; k < nr; k++) {
            const int64_t o = owner[(size_t) (read_first[b] + k)] - read_first[b];
            if (o == k) continue;
            for (int64_t j = 0; j < na; j++) support[support_first[(size_t) b] + j * nr + k] = support[support_first[(size_t) b] + j * nr + o];
        }
    }
    return MRP_OK;
}
int mrp_partition_reads_by_haplotype(mrp_context *ctx, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                     const mrp_haptag_sites *sites, int64_t n_reads, const uint8_t *read_forward_strand, int64_t expansion,
                                     int32_t *hap, double *h1, double *h2, mrp_pairhmm_stats *stats) {
    static const char *who = "mrp_partition_reads_by_haplotype";
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_partition_reads_by_haplotype: no context (the pair-HMM path has no CPU fallback)");
    int rc = ht_check_sites(who, sites, n_reads, read_forward_strand);
    if (rc != MRP_OK) return rc;
    if (!forward_model || !reverse_model || (n_reads > 0 && (!hap || !h1 || !h2))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    if (n_reads == 0) return MRP_OK;
    const mrp_haptag_sites &S = *sites;
    /* heterozygous sites with reads (bubbleGraph.c:1780, :1797-1801) */
    std::vector<uint8_t> active((size_t) S.n_sites);
    for (int64_t s = 0; s < S.n_sites; s++) active[(size_t) s] = S.compare[2 * s] != S.compare[2 * s + 1] && S.entry_first[s + 1] > S.entry_first[s];
    /* b->reads[j] = stList_pop(...) (:1816-1819) reverses the entries, so the cache of :1844-1872 goes to the LAST-listed read
     * with a given substring, and its strand picks the state machine of every duplicate; never anchored (:1832) */
    std::vector<int64_t> owner;
    if (S.n_sites) substring_owners(S.n_sites, S.entry_first, S.pool, S.entry_off, S.entry_len, nullptr, true, owner);
    HtPairs P;
    ht_build_pairs(&S, active, owner, read_forward_strand, INT64_MAX, P);
    if (P.list.size() >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    /* a read's (site, owner pair) list in site order: counting sort by read, filled in site order */
    HostVec<int64_t> first((size_t) n_reads + 1, 0);
    for (int64_t s = 0; s < S.n_sites; s++)
        if (active[(size_t) s])
            for (int64_t k = S.entry_first[s]; k < S.entry_first[s + 1]; k++) first[(size_t) S.entry_read[k] + 1]++;
    for (int64_t r = 0; r < n_reads; r++) first[(size_t) r + 1] += first[(size_t) r];
    HostVec<HtEntry> ent((size_t) first[(size_t) n_reads]);
    {
        std::vector<int64_t> fill(first.begin(), first.end() - 1);
        for (int64_t s = 0; s < S.n_sites; s++) {
            if (!active[(size_t) s]) continue;
            for (int64_t k = S.entry_first[s + 1] - 1; k >= S.entry_first[s]; k--) { /* b->reads order (:1877) */
                const int64_t p = P.pair_of[(size_t) owner[(size_t) k]];
                ent[(size_t) fill[(size_t) S.entry_read[k]]++] = HtEntry{(int32_t) p, (int32_t) p + 1, 0, 0};
            }
        }
    }
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    return phm_call(ctx, who, models, 2, S.pool, S.pool_bytes, P.list.view(), expansion, 0, 0, stats, t_begin, [&](hipStream_t s, const double *lp) {
        DevBuf<int64_t> d_first;
        DevBuf<HtEntry> d_ent;
        DevBuf<int32_t> d_hap;
        DevBuf<double> d_h;
        d_first.pool = d_ent.pool = d_hap.pool = d_h.pool = &ctx->pool;
        PHM_HIP(d_first.upload(first, s));
        PHM_HIP(d_ent.upload(ent, s));
        PHM_HIP(d_hap.alloc((size_t) n_reads));
        PHM_HIP(d_h.alloc(2 * (size_t) n_reads));
        hipLaunchKernelGGL(ht_partition_kernel, dim3((unsigned) ((n_reads + 255) / 256)), dim3(256), 0, s, d_first.p, d_ent.p, lp, n_reads, d_hap.p, d_h.p,
                           d_h.p + n_reads);
        PHM_HIP(hipGetLastError());
        PHM_HIP(hipEventRecord(ctx->ev[1], s));
        PHM_HIP(hipMemcpyAsync(hap, d_hap.p, (size_t) n_reads * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h1, d_h.p, (size_t) n_reads * sizeof(double), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h2, d_h.p + n_reads, (size_t) n_reads * sizeof(double), hipMemcpyDeviceToHost, s));
        return (int) MRP_OK;
    });
}

int mrp_phase_variants_from_tagged_reads(mrp_context *ctx, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                         const mrp_haptag_sites *variants, int64_t n_reads, const uint8_t *read_forward_strand,
                                         const int32_t *read_hap, int64_t expansion, int64_t sv_threshold, int32_t *state, double *cis,
                                         double *trans, mrp_pairhmm_stats *stats) {
    static const char *who = "mrp_phase_variants_from_tagged_reads";
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_phase_variants_from_tagged_reads: no context (the pair-HMM path has no CPU fallback)");
    int rc = ht_check_sites(who, variants, n_reads, read_forward_strand);
    if (rc != MRP_OK) return rc;
    const int64_t n_var = variants->n_sites;
    if (!forward_model || !reverse_model || (n_reads > 0 && !read_hap) || (n_var > 0 && (!state || !cis || !trans)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    if (n_var == 0) return MRP_OK;
    const mrp_haptag_sites &S = *variants;
    const int64_t n_entries = S.entry_first[n_var];
    /* heterozygous variants with reads (bubbleGraph.c:2174, :2186-2192); untagged entries are neither scored nor cached
     * (:2226-2235), so the FIRST tagged entry with a given substring owns the scores */
    std::vector<uint8_t> active((size_t) n_var), tagged((size_t) n_entries);
    for (int64_t v = 0; v < n_var; v++) active[(size_t) v] = S.compare[2 * v] != S.compare[2 * v + 1] && S.entry_first[v + 1] > S.entry_first[v];
    for (int64_t k = 0; k < n_entries; k++) tagged[(size_t) k] = read_hap[S.entry_read[k]] == 1 || read_hap[S.entry_read[k]] == 2;
    std::vector<int64_t> owner;
    substring_owners(n_var, S.entry_first, S.pool, S.entry_off, S.entry_len, tagged.data(), false, owner);
    HtPairs P;
    ht_build_pairs(&S, active, owner, read_forward_strand, sv_threshold, P);
    if (P.list.size() >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    /* a variant's tagged entries in order */
    HostVec<int64_t> first((size_t) n_var + 1, 0);
    HostVec<HtEntry> ent;
    for (int64_t v = 0; v < n_var; v++) {
        if (active[(size_t) v])
            for (int64_t k = S.entry_first[v]; k < S.entry_first[v + 1]; k++) {
                if (!tagged[(size_t) k]) continue;
                const int64_t p = P.pair_of[(size_t) owner[(size_t) k]];
                ent.push_back(HtEntry{(int32_t) p, (int32_t) p + 1, read_hap[S.entry_read[k]] == 1 ? 1 : 0, 0});
            }
        first[(size_t) v + 1] = (int64_t) ent.size();
    }
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    return phm_call(ctx, who, models, 2, S.pool, S.pool_bytes, P.list.view(), expansion, 0, 0, stats, t_begin, [&](hipStream_t s, const double *lp) {
        DevBuf<int64_t> d_first;
        DevBuf<uint8_t> d_active;
        DevBuf<HtEntry> d_ent;
        DevBuf<int32_t> d_state;
        DevBuf<double> d_tot;
        d_first.pool = d_active.pool = d_ent.pool = d_state.pool = d_tot.pool = &ctx->pool;
        PHM_HIP(d_first.upload(first, s));
        PHM_HIP(d_active.upload(active, s));
        PHM_HIP(d_ent.upload(ent, s));
        PHM_HIP(d_state.alloc((size_t) n_var));
        PHM_HIP(d_tot.alloc(2 * (size_t) n_var));
        hipLaunchKernelGGL(ht_phase_kernel, dim3((unsigned) ((n_var + 255) / 256)), dim3(256), 0, s, d_first.p, d_active.p, d_ent.p, lp, n_var, d_state.p,
                           d_tot.p, d_tot.p + n_var);
        PHM_HIP(hipGetLastError());
        PHM_HIP(hipEventRecord(ctx->ev[1], s));
        PHM_HIP(hipMemcpyAsync(state, d_state.p, (size_t) n_var * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(cis, d_tot.p, (size_t) n_var * sizeof(double), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(trans, d_tot.p + n_var, (size_t) n_var * sizeof(double), hipMemcpyDeviceToHost, s));
        return (int) MRP_OK;
    });
}

/* ec_classes_kernel over a host pool: upload, one launch, 4 B per entry back */
int mrp_equal_substring_classes(mrp_context *ctx, int64_t n_sites, const int64_t *entry_first, const uint8_t *pool, int64_t pool_bytes,
                                const int64_t *off, const int32_t *len, int32_t *rep_out) {
    static const char *who = "mrp_equal_substring_classes";
    if (n_sites < 0 || pool_bytes < 0 || !entry_first || (pool_bytes > 0 && !pool)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (entry_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: entry_first must start at 0", who);
    for (int64_t v = 0; v < n_sites; v++)
        if (entry_first[v + 1] < entry_first[v]) return mrp_set_error(MRP_ERR_ARG, "%s: entry_first not ascending at site %lld", who, (long long) v);
    const int64_t n_ent = entry_first[n_sites];
    if (n_ent >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 entries in one call", who);
    if (n_ent > 0 && (!off || !len || !rep_out)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    for (int64_t p = 0; p < n_ent; p++)
        if (len[p] < 0 || off[p] < 0 || off[p] + len[p] > pool_bytes) return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld lies outside the symbol pool", who, (long long) p);
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the classes are found on the device; there is no CPU fallback)", who);
    if (n_ent == 0) return MRP_OK;
    {
        PHM_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DevBuf<uint8_t> d_pool;
        DevBuf<int64_t> d_first, d_off;
        DevBuf<int32_t> d_len, d_rep;
        DevBuf<uint64_t> d_key;
        d_pool.pool = d_first.pool = d_off.pool = d_len.pool = d_rep.pool = d_key.pool = &ctx->pool;
        Drain drain{s};
        PHM_HIP(d_pool.alloc((size_t) pool_bytes));
        PHM_HIP(d_first.alloc((size_t) n_sites + 1));
        PHM_HIP(d_off.alloc((size_t) n_ent));
        PHM_HIP(d_len.alloc((size_t) n_ent));
        PHM_HIP(d_key.alloc((size_t) n_ent));
        PHM_HIP(d_rep.alloc((size_t) n_ent));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_first.p, entry_first, 8 * ((size_t) n_sites + 1), hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_off.p, off, 8 * (size_t) n_ent, hipMemcpyHostToDevice, s));
        PHM_HIP(hipMemcpyAsync(d_len.p, len, 4 * (size_t) n_ent, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ec_classes_kernel<int32_t>, dim3((unsigned) std::min<int64_t>(n_sites, 65536)), dim3(PHM_WAVE), 0, s, d_first.p, n_sites, d_len.p,
                           d_off.p, d_pool.p, d_key.p, d_rep.p);
        PHM_HIP(hipGetLastError());
        HostVec<int32_t> rep((size_t) n_ent); /* (rep_out is written only on success) */
        PHM_HIP(hipMemcpyAsync(rep.data(), d_rep.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipStreamSynchronize(s));
        memcpy(rep_out, rep.data(), 4 * (size_t) n_ent);
    }
    ctx->pool.reclaim();
    return MRP_OK;
}

}  // extern "C"

/* ---- mrp_phase_string_chunks in three steps (mrp_internal.h): its own body below, and what a lane of the work queue runs per
 * batch (mrp_queue.cpp) -- the checks of every chunk first, the front of batch n + 1 beside the device work of batch n. */

struct mrp_string_front {
    int64_t n_chunks = 0, n_subs = 0, n_pairs = 0;
    const mrp_string_chunk *chunks = nullptr;          /* the caller's, alive until the run has returned */
    std::vector<int64_t> pool_base, sub_base;          /* n_chunks + 1: chunk c's symbols and substrings in the call's arrays */
    HostVec<uint8_t> gpool;                            /* every chunk's symbols: what the pair-HMM kernels read */
    const uint8_t *device_pool = nullptr;              /* set (mrp_phase_aligned_chunks): the symbols lie in HBM already, device_pool_bytes of */
    int64_t device_pool_bytes = 0;                     /* them, written by work queued on the run's stream; gpool is empty and not read */
    std::vector<int64_t> pair_first;                   /* per substring: the pair of its owner with the bubble's allele 0 */
    PhmLaunch L;                                       /* the pairs as phm_classify sorted them; the run adds the device half (PhmDev) */
    /* what only the front itself reads, kept until the front is destroyed: released between front and run, these ~100 bytes per
     * pair go back to the system and the run's own arrays fault fresh pages in (12 chunks of 2 000 sites: a call of 68-77 ms
     * instead of 56-61) */
    struct Scratch {
        std::vector<int64_t> g_sub_first, g_sub_off, owner;
        std::vector<int32_t> g_sub_len;
        PhmPairList pairs;                             /* the front's own, then the back half's speculative ones */
        std::vector<std::vector<int64_t>> chunk_anchors;
        /* a front over a device pool with a rest (mrp_phase_aligned_chunks_with_filtered): the host has no symbol, so the classes of equal
         * substrings come as ids (ec_classes_kernel: equal ids at a site = equal substrings) -- per substring of the call, per chunk per
         * fsub / ventry of its rest -- and the back half's pairs that want k-mer anchors are listed for the anchors kernel */
        bool classes_by_id = false;
        std::vector<int64_t> sub_cls;
        std::vector<std::vector<int64_t>> fsub_cls, ventry_cls;
        std::vector<int64_t> anchored_new;
    } scratch;
    double front_ms = 0;                               /* host wall time of the front (the one call adds its checks) */
    /* the back half (a call with rests): the static part of its sites, made with the pairs.  Sites: the bubbles of the chunks
     * with a rest, chunk by chunk, then the variants, chunk by chunk. */
    struct Filtered {
        bool on = false;
        const mrp_string_chunk_rest *rest = nullptr;   /* the caller's, as chunks */
        std::vector<int64_t> read_base, var_base;      /* n_chunks + 1: chunk c's reads (primary, then filtered) and variants in the call */
        int64_t n_bsites = 0, n_primary_pairs = 0;
        HostVec<FsEntry> entries;
        HostVec<FsSite> sites;
        HostVec<int32_t> cbase, pidx;
        HostVec<int64_t> cand_first;                   /* per read of the call: its entries at bubbles, in bubble order */
        HostVec<int32_t> cand;
    } fil;
};

int mrp_string_chunks_check(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                            int64_t expansion, const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                            const mrp_string_chunk_rest *rest, const char *who) {
    if (n_chunks < 0 || (n_chunks > 0 && (!chunks || !out || !hap_out)) || !forward_model || !reverse_model || !params)
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    for (int64_t c = 0; c < n_chunks; c++)
        if (chunks[c].n_reads > 0 && (!hap_out[c] || (phred_out && !phred_out[c]))) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output", who, (long long) c);
    {
        std::vector<int> rcs((size_t) n_chunks, MRP_OK);
        std::vector<std::string> msgs((size_t) n_chunks);
        mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
            std::vector<int64_t> seen;
            rcs[(size_t) c] = sc_check_chunk(who, c, chunks[c], seen);
            if (rcs[(size_t) c] == MRP_OK && rest) rcs[(size_t) c] = sc_check_rest(who, c, chunks[c], rest[c]);
            if (rcs[(size_t) c] != MRP_OK) msgs[(size_t) c] = mrp_last_error();
        });
        for (int64_t c = 0; c < n_chunks; c++)
            if (rcs[(size_t) c] != MRP_OK) return mrp_set_error(rcs[(size_t) c], "%s", msgs[(size_t) c].c_str());
    }
    return MRP_OK;
}

/* MRP_ERR_UNSUPPORTED as phm_classify raises it, from the strings alone -- without the owners, the pair list or the sort (a
 * duplicate substring has its owner's strings, so looking at every substring changes nothing).  A diagonal of a pair holds at
 * most min(lx, ly) + 1 cells, band or not: only pairs with BOTH strings at the limit are looked at, their anchors (above
 * sv_threshold, bubbleGraph.c:1448-1451) and bands made as the front makes them. */
int mrp_string_chunks_check_pairs(int64_t n_chunks, const mrp_string_chunk *chunks, int64_t expansion, int64_t sv_threshold,
                                  const mrp_string_chunk_rest *rest, const char *who) {
    std::vector<int> rcs((size_t) n_chunks, MRP_OK);
    std::vector<std::string> msgs((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        std::vector<int64_t> anc;
        std::vector<int32_t> Lb, Rb;
        int &rcc = rcs[(size_t) c];
        /* one pair: x = allele, y = substring; what: "bubble" / "variant" and its index.  Leaves rcc set on a refusal. */
        auto pair = [&](const uint8_t *x, int64_t lx, const uint8_t *y, int64_t ly, bool anchored, const char *what, int64_t idx) {
            if (std::min(lx, ly) < PHM_WAVE_MAX_WIDTH) return;
            anc.clear();
            if (anchored) kmer_anchors(x, lx, y, ly, anc);
            int width = (int) std::min<int64_t>(std::min(lx, ly) + 1, INT32_MAX);
            if (!anc.empty()) {
                if (lx + ly >= (1ll << 30)) { rcc = mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who); return; }
                Lb.resize((size_t) (lx + ly + 1));
                Rb.resize((size_t) (lx + ly + 1));
                const int rc = band_closed_form(anc.data(), (int64_t) anc.size() / 2, lx, ly, expansion, Lb.data(), Rb.data(), nullptr, &width);
                if (rc != MRP_OK) {
                    rcc = mrp_set_error(rc, "%s: chunk %lld: a pair of %s %lld has invalid anchors (pairwiseAligner.c:206-211)", who, (long long) c, what, (long long) idx);
                    return;
                }
            }
            if (width > PHM_WAVE_MAX_WIDTH)
                rcc = mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: chunk %lld: a pair of %s %lld has a diagonal of %d cells (limit %d)", who, (long long) c, what,
                                    (long long) idx, width, PHM_WAVE_MAX_WIDTH);
        };
        for (int64_t b = 0; b < S.n_bubbles && rcc == MRP_OK; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1] && rcc == MRP_OK; k++)
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1] && rcc == MRP_OK; j++)
                    pair(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], S.sub_len[k] > sv_threshold || S.allele_len[j] > sv_threshold,
                         "bubble", b);
        if (rest && !sc_rest_empty(rest[c])) {
            /* the back half's pairs: every substring of a bubble, primary or filtered, against every allele without anchors (the
             * partition never anchors, bubbleGraph.c:1832); a variant's entries of primary reads against its two gt alleles */
            const mrp_string_chunk_rest &R = rest[c];
            for (int64_t b = 0; b < S.n_bubbles && rcc == MRP_OK; b++)
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1] && rcc == MRP_OK; j++) {
                    for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1] && rcc == MRP_OK; k++)
                        pair(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], false, "bubble", b);
                    for (int64_t k = R.fsub_first ? R.fsub_first[b] : 0; k < (R.fsub_first ? R.fsub_first[b + 1] : 0) && rcc == MRP_OK; k++)
                        pair(S.pool + S.allele_off[j], S.allele_len[j], R.pool + R.fsub_off[k], R.fsub_len[k], false, "bubble", b);
                }
            for (int64_t v = 0; v < R.n_variants && rcc == MRP_OK; v++) {
                if (R.gt[2 * v] == R.gt[2 * v + 1]) continue;
                for (int64_t k = R.ventry_first[v]; k < R.ventry_first[v + 1] && rcc == MRP_OK; k++) {
                    if (R.ventry_read[k] >= S.n_reads) continue;
                    for (int w = 0; w < 2 && rcc == MRP_OK; w++) {
                        const int64_t j = R.valle_first[v] + R.gt[2 * v + w];
                        pair(R.pool + R.valle_off[j], R.valle_len[j], R.pool + R.ventry_off[k], R.ventry_len[k],
                             R.ventry_len[k] > sv_threshold || R.valle_len[j] > sv_threshold, "variant", v);
                    }
                }
            }
        }
        if (rcc != MRP_OK) msgs[(size_t) c] = mrp_last_error();
    });
    for (int64_t c = 0; c < n_chunks; c++)
        if (rcs[(size_t) c] != MRP_OK) return mrp_set_error(rcs[(size_t) c], "%s", msgs[(size_t) c].c_str());
    return MRP_OK;
}

void mrp_string_front_destroy(mrp_string_front *F) { delete F; }

/* The static half of the back half, made with the front (host only): per chunk with a rest its sites (bubbles, then variants), their
 * entries grouped into classes of equal substrings (the sort of substring_owners), and one pair per (class, strand that occurs in
 * the class, allele) some outcome of the phasing could read -- for a bubble every allele, never anchored; for a variant its two gt
 * alleles, anchored past sv_threshold, and only classes and strands of primary reads (a filtered read is never tagged).  A pair
 * the front already scores (same substring, same strand's model, not anchored) is referred to, not added.  The new pairs go behind
 * the front's own in its pair list. */
struct FsLocal { /* one task's share; pidx: a pair of the front (>= 0) or ~(index among the task's new pairs) */
    std::vector<FsEntry> entries;
    std::vector<FsSite> bsites, vsites;
    std::vector<int32_t> cbase;
    std::vector<int64_t> pidx;
    PhmPairList pairs;
    std::vector<int64_t> anchored; /* classes by id: the new pairs past sv_threshold, whose anchors are found on the device */
};
/* a task: a run of bubbles or of variants of one chunk (a chunk of 2 000 sites is sixteen tasks, not one) */
struct FsTask { int64_t c; bool variants; int64_t lo, hi; };

static void sc_filtered_task(const mrp_string_front *F, const mrp_string_chunk_rest *rest, int64_t sv_threshold, const std::vector<int64_t> &rpool_base,
                             const FsTask &T, FsLocal &Lc) {
    const mrp_string_front::Scratch &X = F->scratch;
    const uint8_t *gpool = F->gpool.data();
    const int64_t c = T.c;
    const mrp_string_chunk &S = F->chunks[c];
    const mrp_string_chunk_rest &R = rest[c];
    const int64_t pb = F->pool_base[(size_t) c], rb = rpool_base[(size_t) c], sb = F->sub_base[(size_t) c];
    const bool by_id = X.classes_by_id; /* the symbols lie in HBM: equal substrings of a site carry equal ids */
    struct Item { int64_t off; int32_t len; int64_t prim_sub; bool may_own; int64_t id; };
    std::vector<Item> items;
    std::vector<int32_t> order;
    auto same = [&](int32_t a, int32_t d) {
        const Item &x = items[(size_t) a], &y = items[(size_t) d];
        return by_id ? x.id == y.id : x.len == y.len && memcmp(gpool + x.off, gpool + y.off, (size_t) x.len) == 0;
    };
    /* classes of the items that may own (entries [e0, e0 + items.size()) of Lc.entries); per class and strand block(cls, rev, rep):
     * adds the (class, strand)'s pairs and returns where its block starts in Lc.pidx */
    auto classes = [&](size_t e0, FsSite &st, auto block) {
        order.clear();
        for (size_t i = 0; i < items.size(); i++)
            if (items[i].may_own) order.push_back((int32_t) i);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t d) {
            const Item &x = items[(size_t) a], &y = items[(size_t) d];
            if (by_id) return x.id != y.id ? x.id < y.id : a < d; /* (another numbering of the classes: only the order of the pairs differs) */
            if (x.len != y.len) return x.len < y.len;
            const int cmp = memcmp(gpool + x.off, gpool + y.off, (size_t) x.len);
            return cmp != 0 ? cmp < 0 : a < d;
        });
        st.cls_first = (int64_t) Lc.cbase.size() / 2;
        int32_t n_cls = 0;
        for (size_t i = 0; i < order.size(); n_cls++) {
            size_t j = i + 1;
            while (j < order.size() && same(order[i], order[j])) j++;
            int64_t prim = -1;
            bool has[2] = {false, false};
            for (size_t q = i; q < j; q++) {
                FsEntry &e = Lc.entries[e0 + (size_t) order[q]];
                e.cls = n_cls;
                has[e.flags & 1] = true;
                if (prim < 0) prim = items[(size_t) order[q]].prim_sub;
            }
            for (int rev = 0; rev < 2; rev++) Lc.cbase.push_back(has[rev] ? (int32_t) block(rev, items[(size_t) order[i]], prim) : -1);
            i = j;
        }
        st.n_classes = n_cls;
    };
    auto new_pair = [&](int64_t xo, int32_t xl, int64_t yo, int32_t yl, int rev, bool anchored) {
        Lc.pidx.push_back(~Lc.pairs.size());
        if (anchored && by_id) Lc.anchored.push_back(Lc.pairs.size());
        Lc.pairs.add(xo, xl, yo, yl, rev, anchored && !by_id ? gpool : nullptr);
    };
    for (int64_t b = T.variants ? T.hi : T.lo; b < T.hi; b++) {
        FsSite st{};
        st.entry_first = (int64_t) Lc.entries.size();
        st.chunk = (int32_t) c;
        st.bubble = (int32_t) b;
        st.n_alleles = (int32_t) (S.allele_first[b + 1] - S.allele_first[b]);
        st.visited = 1;
        items.clear();
        /* listing order of the partition: the filtered reads in index order, then the primary reads in index order */
        for (int64_t k = R.fsub_first ? R.fsub_first[b] : 0; k < (R.fsub_first ? R.fsub_first[b + 1] : 0); k++) {
            const int32_t fr = R.fsub_read[k];
            Lc.entries.push_back(FsEntry{0, (int32_t) (S.n_reads + fr), fr, (R.forward_strand[fr] ? 0 : 1) | 2});
            items.push_back(Item{rb + R.fsub_off[k], R.fsub_len[k], -1, true, by_id ? X.fsub_cls[(size_t) c][(size_t) k] : -1});
        }
        for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
            const int32_t r = S.sub_read[k];
            Lc.entries.push_back(FsEntry{0, r, (int32_t) (R.n_filtered + r), S.read_forward_strand[r] ? 0 : 1});
            items.push_back(Item{pb + S.sub_off[k], S.sub_len[k], sb + k, true, by_id ? X.sub_cls[(size_t) (sb + k)] : -1});
        }
        st.n_entries = (int32_t) items.size();
        classes((size_t) st.entry_first, st, [&](int rev, const Item &rep, int64_t prim) {
            const int64_t at = (int64_t) Lc.pidx.size();
            /* the front's own pairs of this substring: its owner's strand, anchored past sv_threshold (bubbleGraph.c:1448-1451) */
            int prim_rev = -1;
            if (prim >= 0) {
                const int64_t po = X.owner[(size_t) prim] - sb;
                prim_rev = S.read_forward_strand[S.sub_read[po]] ? 0 : 1;
            }
            for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1]; j++) {
                if (prim_rev == rev && !(rep.len > sv_threshold || S.allele_len[j] > sv_threshold))
                    Lc.pidx.push_back(F->pair_first[(size_t) prim] + (j - S.allele_first[b]));
                else
                    new_pair(pb + S.allele_off[j], S.allele_len[j], rep.off, rep.len, rev, false);
            }
            return at;
        });
        Lc.bsites.push_back(st);
    }
    for (int64_t v = T.variants ? T.lo : T.hi; v < T.hi; v++) {
        FsSite st{};
        st.entry_first = (int64_t) Lc.entries.size();
        st.chunk = (int32_t) c;
        st.bubble = -1;
        st.n_alleles = 2;
        st.n_entries = (int32_t) (R.ventry_first[v + 1] - R.ventry_first[v]);
        st.visited = R.gt[2 * v] != R.gt[2 * v + 1] && st.n_entries > 0;
        items.clear();
        for (int64_t k = R.ventry_first[v]; k < R.ventry_first[v + 1]; k++) {
            const int32_t r = R.ventry_read[k];
            const bool filtered = r >= S.n_reads;
            const bool fwd = filtered ? R.forward_strand[r - S.n_reads] != 0 : S.read_forward_strand[r] != 0;
            Lc.entries.push_back(FsEntry{0, r, (int32_t) (k - R.ventry_first[v]), (fwd ? 0 : 1) | (filtered ? 2 : 0)});
            items.push_back(Item{rb + R.ventry_off[k], R.ventry_len[k], -1, st.visited && !filtered, by_id ? X.ventry_cls[(size_t) c][(size_t) k] : -1});
        }
        classes((size_t) st.entry_first, st, [&](int rev, const Item &rep, int64_t) {
            const int64_t at = (int64_t) Lc.pidx.size();
            for (int w = 0; w < 2; w++) {
                const int64_t j = R.valle_first[v] + R.gt[2 * v + w];
                new_pair(rb + R.valle_off[j], R.valle_len[j], rep.off, rep.len, rev, rep.len > sv_threshold || R.valle_len[j] > sv_threshold); /* bubbleGraph.c:2253-2263 */
            }
            return at;
        });
        Lc.vsites.push_back(st);
    }
}

static int sc_filtered_front(mrp_string_front *F, const mrp_string_chunk_rest *rest, int64_t sv_threshold, const std::vector<int64_t> &rpool_base) {
    static const char *who = "mrp_phase_string_chunks_with_filtered";
    const int64_t n_chunks = F->n_chunks;
    const mrp_string_chunk *chunks = F->chunks;
    mrp_string_front::Filtered &Q = F->fil;
    mrp_string_front::Scratch &X = F->scratch;
    Q.on = true;
    Q.rest = rest;
    Q.n_primary_pairs = F->n_pairs;
    Q.read_base.assign((size_t) n_chunks + 1, 0);
    Q.var_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        Q.read_base[(size_t) c + 1] = Q.read_base[(size_t) c] + chunks[c].n_reads + rest[c].n_filtered;
        Q.var_base[(size_t) c + 1] = Q.var_base[(size_t) c] + rest[c].n_variants;
    }
    if (Q.read_base[(size_t) n_chunks] >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 reads in one call", who);
    std::vector<FsTask> tasks;
    constexpr int64_t TASK_SITES = 128;
    for (int64_t c = 0; c < n_chunks; c++) {
        if (sc_rest_empty(rest[c])) continue;
        for (int64_t lo = 0; lo < chunks[c].n_bubbles; lo += TASK_SITES) tasks.push_back(FsTask{c, false, lo, std::min(chunks[c].n_bubbles, lo + TASK_SITES)});
        for (int64_t lo = 0; lo < rest[c].n_variants; lo += TASK_SITES) tasks.push_back(FsTask{c, true, lo, std::min(rest[c].n_variants, lo + TASK_SITES)});
    }
    std::vector<FsLocal> loc(tasks.size());
    mrp_parallel_for((int64_t) tasks.size(), 1, [&](int64_t ti) { sc_filtered_task(F, rest, sv_threshold, rpool_base, tasks[(size_t) ti], loc[(size_t) ti]); });
    /* ---- side by side: entries, class tables and blocks task by task; the sites as bubbles of every chunk, then variants */
    int64_t n_entries = 0, n_cbase = 0, n_pidx = 0, n_new = 0, n_b = 0, n_v = 0;
    for (const FsLocal &Lc : loc) {
        n_entries += (int64_t) Lc.entries.size(); n_cbase += (int64_t) Lc.cbase.size(); n_pidx += (int64_t) Lc.pidx.size(); n_new += Lc.pairs.size();
        n_b += (int64_t) Lc.bsites.size(); n_v += (int64_t) Lc.vsites.size();
    }
    if (F->n_pairs + n_new >= (1ll << 31) || n_entries >= (1ll << 31) || n_pidx >= (1ll << 31) || n_cbase >= (1ll << 31) || n_b + n_v >= (1ll << 31))
        return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs or entries in one call", who);
    Q.entries.resize((size_t) n_entries);
    Q.cbase.resize((size_t) n_cbase);
    Q.pidx.resize((size_t) n_pidx);
    Q.sites.resize((size_t) (n_b + n_v));
    Q.n_bsites = n_b;
    int64_t e0 = 0, c0 = 0, p0 = 0, b0 = 0, v0 = n_b, pair0 = F->n_pairs;
    for (size_t ti = 0; ti < tasks.size(); ti++) {
        const FsLocal &Lc = loc[ti];
        const int64_t c = tasks[ti].c;
        for (size_t i = 0; i < Lc.entries.size(); i++) {
            FsEntry e = Lc.entries[i];
            e.read += (int32_t) Q.read_base[(size_t) c];
            Q.entries[(size_t) e0 + i] = e;
        }
        for (size_t i = 0; i < Lc.cbase.size(); i++) Q.cbase[(size_t) c0 + i] = Lc.cbase[i] < 0 ? -1 : Lc.cbase[i] + (int32_t) p0;
        for (size_t i = 0; i < Lc.pidx.size(); i++) Q.pidx[(size_t) p0 + i] = (int32_t) (Lc.pidx[i] >= 0 ? Lc.pidx[i] : pair0 + ~Lc.pidx[i]);
        for (const FsSite &st : Lc.bsites) { FsSite g = st; g.entry_first += e0; g.cls_first += c0 / 2; Q.sites[(size_t) b0++] = g; }
        for (const FsSite &st : Lc.vsites) { FsSite g = st; g.entry_first += e0; g.cls_first += c0 / 2; Q.sites[(size_t) v0++] = g; }
        for (int64_t q : Lc.anchored) X.anchored_new.push_back(pair0 + q);
        X.pairs.append(Lc.pairs);
        e0 += (int64_t) Lc.entries.size(); c0 += (int64_t) Lc.cbase.size(); p0 += (int64_t) Lc.pidx.size(); pair0 += Lc.pairs.size();
    }
    F->n_pairs = pair0;
    /* a read's entries at bubbles in bubble order (a counting sort by read, filled in site order) */
    const int64_t n_reads_all = Q.read_base[(size_t) n_chunks];
    Q.cand_first.assign((size_t) n_reads_all + 1, 0);
    for (int64_t s = 0; s < n_b; s++)
        for (int64_t i = Q.sites[(size_t) s].entry_first; i < Q.sites[(size_t) s].entry_first + Q.sites[(size_t) s].n_entries; i++)
            Q.cand_first[(size_t) Q.entries[(size_t) i].read + 1]++;
    for (int64_t r = 0; r < n_reads_all; r++) Q.cand_first[(size_t) r + 1] += Q.cand_first[(size_t) r];
    Q.cand.resize((size_t) Q.cand_first[(size_t) n_reads_all]);
    std::vector<int64_t> fill(Q.cand_first.begin(), Q.cand_first.end() - 1);
    for (int64_t s = 0; s < n_b; s++)
        for (int64_t i = Q.sites[(size_t) s].entry_first; i < Q.sites[(size_t) s].entry_first + Q.sites[(size_t) s].n_entries; i++)
            Q.cand[(size_t) fill[(size_t) Q.entries[(size_t) i].read]++] = (int32_t) i;
    return MRP_OK;
}

int mrp_string_front_create(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest, const mrp_pair_hmm *forward_model,
                            const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, mrp_string_front **front_out) {
    const char *who = rest ? "mrp_phase_string_chunks_with_filtered" : "mrp_phase_string_chunks";
    const double t_begin = now_ms();
    *front_out = nullptr;
    mrp_string_front *F = new (std::nothrow) mrp_string_front();
    if (!F) return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks: out of host memory");
    struct Drop { mrp_string_front *f; ~Drop() { delete f; } } drop{F}; /* (an early return) */
    F->n_chunks = n_chunks;
    F->chunks = chunks;
    /* ---- the pairs of every chunk, one symbol pool: bubble b of chunk c is global bubble bubble_base[c] + b */
    std::vector<int64_t> &pool_base = F->pool_base, &sub_base = F->sub_base, bubble_base((size_t) n_chunks + 1, 0);
    pool_base.assign((size_t) n_chunks + 1, 0);
    sub_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        pool_base[(size_t) c + 1] = pool_base[(size_t) c] + chunks[c].pool_bytes;
        bubble_base[(size_t) c + 1] = bubble_base[(size_t) c] + chunks[c].n_bubbles;
        sub_base[(size_t) c + 1] = sub_base[(size_t) c] + (chunks[c].n_bubbles ? chunks[c].sub_first[chunks[c].n_bubbles] : 0);
    }
    const int64_t n_bub = bubble_base[(size_t) n_chunks], n_subs = sub_base[(size_t) n_chunks];
    HostVec<uint8_t> &gpool = F->gpool;
    /* the rests' symbols behind the chunks' (a rest that points at its chunk's pool reads it there) */
    std::vector<int64_t> rpool_base((size_t) n_chunks, 0);
    int64_t gpool_bytes = pool_base[(size_t) n_chunks];
    auto rest_has_own_pool = [&](int64_t c) { return !(rest[c].pool == chunks[c].pool && rest[c].pool_bytes == chunks[c].pool_bytes); };
    if (rest)
        for (int64_t c = 0; c < n_chunks; c++) {
            rpool_base[(size_t) c] = pool_base[(size_t) c];
            if (sc_rest_empty(rest[c]) || !rest_has_own_pool(c)) continue;
            rpool_base[(size_t) c] = gpool_bytes;
            gpool_bytes += rest[c].pool_bytes;
        }
    gpool.resize((size_t) gpool_bytes);
    mrp_string_front::Scratch &X = F->scratch;
    std::vector<int64_t> &g_sub_first = X.g_sub_first, &g_sub_off = X.g_sub_off;
    std::vector<int32_t> &g_sub_len = X.g_sub_len;
    g_sub_first.assign((size_t) n_bub + 1, 0);
    g_sub_off.resize((size_t) n_subs);
    g_sub_len.resize((size_t) n_subs);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        if (S.pool_bytes) memcpy(gpool.data() + pool_base[(size_t) c], S.pool, (size_t) S.pool_bytes);
        if (rest && !sc_rest_empty(rest[c]) && rest_has_own_pool(c) && rest[c].pool_bytes)
            memcpy(gpool.data() + rpool_base[(size_t) c], rest[c].pool, (size_t) rest[c].pool_bytes);
        for (int64_t b = 0; b < S.n_bubbles; b++) g_sub_first[(size_t) (bubble_base[(size_t) c] + b + 1)] = sub_base[(size_t) c] + S.sub_first[b + 1];
        const int64_t ns = sub_base[(size_t) c + 1] - sub_base[(size_t) c];
        for (int64_t k = 0; k < ns; k++) {
            g_sub_off[(size_t) (sub_base[(size_t) c] + k)] = pool_base[(size_t) c] + S.sub_off[k];
            g_sub_len[(size_t) (sub_base[(size_t) c] + k)] = S.sub_len[k];
        }
    });
    /* cachedScores (bubbleGraph.c:1418,1431-1441): the first substring of the bubble with given symbols owns the scores */
    std::vector<int64_t> &owner = X.owner;
    substring_owners(n_bub, g_sub_first.data(), gpool.data(), g_sub_off.data(), g_sub_len.data(), nullptr, false, owner);
    /* the owners' pairs, chunk by chunk in parallel: pair_first[k] = the pair of owner k with the bubble's allele 0 */
    std::vector<int64_t> pair_base((size_t) n_chunks + 1, 0), &pair_first = F->pair_first;
    pair_first.assign((size_t) n_subs, -1);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_string_chunk &S = chunks[c];
        int64_t np = 0;
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++)
                if (owner[(size_t) (sub_base[(size_t) c] + k)] == sub_base[(size_t) c] + k) np += S.allele_first[b + 1] - S.allele_first[b];
        pair_base[(size_t) c + 1] = pair_base[(size_t) c] + np;
    }
    const int64_t n_pairs = pair_base[(size_t) n_chunks];
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    PhmPairList &pairs = X.pairs;
    std::vector<std::vector<int64_t>> &chunk_anchors = X.chunk_anchors;
    pairs.resize(n_pairs);
    chunk_anchors.resize((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        const int64_t pb = pool_base[(size_t) c], sb = sub_base[(size_t) c];
        int64_t p = pair_base[(size_t) c];
        std::vector<int64_t> &anc = chunk_anchors[(size_t) c];
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
                if (owner[(size_t) (sb + k)] != sb + k) continue;
                pair_first[(size_t) (sb + k)] = p;
                for (int64_t j = S.allele_first[b]; j < S.allele_first[b + 1]; j++, p++) {
                    const size_t before = anc.size();
                    if (S.sub_len[k] > sv_threshold || S.allele_len[j] > sv_threshold) /* bubbleGraph.c:1448-1451 */
                        kmer_anchors(S.pool + S.allele_off[j], S.allele_len[j], S.pool + S.sub_off[k], S.sub_len[k], anc);
                    pairs.set(p, pb + S.allele_off[j], S.allele_len[j], pb + S.sub_off[k], S.sub_len[k], S.read_forward_strand[S.sub_read[k]] ? 0 : 1,
                              (int64_t) (anc.size() - before) / 2);
                }
            }
    });
    pairs.counts_to_offsets();
    for (auto &v : chunk_anchors) pairs.anchors.insert(pairs.anchors.end(), v.begin(), v.end());
    for (int64_t k = 0; k < n_subs; k++) /* duplicates read their owner's pairs */
        if (owner[(size_t) k] != k) pair_first[(size_t) k] = pair_first[(size_t) owner[(size_t) k]];

    F->n_subs = n_subs;
    F->n_pairs = n_pairs;
    if (rest) { /* the back half's sites; its speculative pairs join the list behind the front's own */
        const int rc = sc_filtered_front(F, rest, sv_threshold, rpool_base);
        if (rc != MRP_OK) return rc;
    }
    if (F->n_pairs > 0) {
        const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
        const int rc = phm_classify(who, models, 2, (int64_t) gpool.size(), pairs.view(), expansion, 0, 0, F->L);
        if (rc != MRP_OK) return rc;
    }
    F->front_ms = now_ms() - t_begin;
    drop.f = nullptr;
    *front_out = F;
    return MRP_OK;
}

namespace {

static void *sc_dup(const void *src, size_t bytes) { /* a result array the caller frees with mrp_free */
    void *p = malloc(bytes ? bytes : 1);
    if (p && bytes) memcpy(p, src, bytes);
    return p;
}

/* One run of a front: everything the queued work reads or writes until the stream has drained -- the stream, the device and pinned
 * buffers, the host sources of the uploads, the events, the layouts -- and the chunks and results that are the run's until it hands
 * them over.  The destructor drains the stream first, then deletes the chunks and whatever was not handed over; the buffers' own
 * destructors follow, so mrp_string_front_run reclaims the pool once the ScRun is gone and no block can be forgotten.
 * The steps run in the order mrp_string_front_run lists them; each queues its work on ctx->stream in the order written. */
struct ScRun {
    mrp_context *const ctx;
    mrp_string_front *const F;
    mrp_string_chunks_stats *const stats;
    mrp_string_filtered_stats *const filtered_stats;
    const int64_t n_chunks, n_subs, n_pairs;
    const mrp_string_chunk *const chunks;
    hipStream_t s = nullptr; /* set once the device is current: from then on the destructor drains it */
    enum { EV_PAIRS_END, EV_BYTES_BEGIN, EV_BYTES_END, EV_POOL_HOME, EV_TAGS_BEGIN, EV_BACK_BEGIN, EV_BACK_END, N_EV };
    hipEvent_t ev[N_EV] = {};
    PhmDev D; /* the pair-HMM's device half: D.d_out holds the log probabilities every later kernel reads */
    DevBuf<ScByteItem> d_items;
    DevBuf<uint8_t> d_pool;
    DevBuf<int64_t> d_aoff;
    DevBuf<uint64_t> d_haps;
    DevBuf<ScHapItem> d_hitems;
    DevBuf<int8_t> d_hap;
    DevBuf<double> d_phred;
    PinnedBuf h_pool, h_res;
    int8_t *h_hap = nullptr;
    double *h_phred = nullptr;
    std::vector<ScLayout> lay;
    std::vector<int64_t> dpool_base, aoff_base, seq_base, hap_base; /* n_chunks + 1: chunk c's share of the call's arrays */
    int64_t dpool_bytes = 0, n_seqs_all = 0;
    HostVec<ScByteItem> items;
    HostVec<int64_t> aoff_all;
    HostVec<uint64_t> haps;
    HostVec<ScHapItem> hitems;
    mrp_chunk_block blk;
    std::vector<mrp_chunk *> dch;
    std::vector<mrp_phase_result *> res;
    double phase_ms = 0; /* host wall time inside mrp_phase_reads_many */

    /* The back half's share: its static tables, what the phasing decided per chunk, a record per entry, the results.
     * Its four methods are called where the run has the matching step of its own; `on` false makes each a no-op. */
    struct Back {
        const mrp_string_front::Filtered &Q;
        mrp_filtered_out *const out;
        const bool on, count_used;
        int64_t n_reads = 0, n_vars = 0;
        size_t n_tot = 0, n_i32 = 0;
        DevBuf<FsEntry> d_ent;
        DevBuf<FsSite> d_sites;
        DevBuf<FsChunk> d_chunks;
        DevBuf<int32_t> d_cbase, d_pidx, d_cand, d_read_seq, d_hap;
        DevBuf<int64_t> d_cand_first;
        DevBuf<HtEntry> d_rec;
        DevBuf<double> d_tot;
        DevBuf<uint8_t> d_used;
        HostVec<int32_t> read_seq;
        HostVec<FsChunk> fchunks;
        PinnedBuf h_res;
        double *h_tot = nullptr;
        int32_t *h_hap = nullptr;
        uint8_t *h_used = nullptr;
        float ms = 0.f;
        Back(const mrp_string_front::Filtered &q, mrp_filtered_out *o, bool stats) : Q(q), out(o), on(q.on && o != nullptr), count_used(on && stats) {}
        void bind(DevPool *pl) {
            d_ent.pool = d_sites.pool = d_chunks.pool = d_cbase.pool = d_pidx.pool = d_cand.pool = d_read_seq.pool = d_hap.pool = d_cand_first.pool =
                d_rec.pool = d_tot.pool = d_used.pool = pl;
        }
        int upload_static(ScRun &R);
        int alloc_results(ScRun &R);
        int launch(ScRun &R);
        int hand_over(ScRun &R, mrp_profile_out *profiles_out);
    } back;

    ScRun(mrp_context *c, mrp_string_front *f, mrp_string_chunks_stats *st, mrp_filtered_out *filtered_out, mrp_string_filtered_stats *fst)
        : ctx(c), F(f), stats(st), filtered_stats(fst), n_chunks(f->n_chunks), n_subs(f->n_subs), n_pairs(f->n_pairs), chunks(f->chunks),
          dch((size_t) f->n_chunks, nullptr), res((size_t) f->n_chunks, nullptr), back(f->fil, filtered_out, fst != nullptr) {
        /* the one place that binds the run's device buffers to the context's pool (D: phm_enqueue) */
        d_items.pool = d_pool.pool = d_aoff.pool = d_haps.pool = d_hitems.pool = d_hap.pool = d_phred.pool = &ctx->pool;
        back.bind(&ctx->pool);
    }
    ~ScRun() {
        if (s) (void) hipStreamSynchronize(s);
        for (mrp_chunk *ch : dch) delete ch;
        for (mrp_phase_result *r : res) mrp_phase_result_destroy(r);
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
    }
    int begin();
    int enqueue_pairhmm();
    int layout_and_items(double het_substitution_probability);
    int profile_bytes();
    int chunks_and_phase(const mrp_params *params);
    int hp_tags(int64_t min_phred);
    int download();
    int hand_over(mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out);
};

int ScRun::begin() {
    PHM_HIP(hipSetDevice(ctx->device));
    s = ctx->stream;
    for (hipEvent_t &x : ev) PHM_HIP(hipEventCreate(&x));
    return MRP_OK;
}

/* the pair-HMM kernels over the front's launch classes; EV_PAIRS_END behind them */
int ScRun::enqueue_pairhmm() {
    if (n_pairs > 0) {
        const int64_t pool_bytes = F->device_pool ? F->device_pool_bytes : (int64_t) F->gpool.size();
        const int rc = phm_enqueue(ctx, F->gpool.data(), pool_bytes, n_pairs, F->L, D, stats ? &stats->pairhmm : nullptr, F->device_pool);
        if (rc != MRP_OK) return rc;
    } else {
        PHM_HIP(hipEventRecord(ctx->ev[0], s));
    }
    PHM_HIP(hipEventRecord(ev[EV_PAIRS_END], s));
    return MRP_OK;
}

/* on the host, beside the pair-HMM kernels: the layout of every chunk (the index arrays only) and where each (bubble, substring)'s
 * bytes go.  Every chunk's pool lies in one device buffer, with mrp_chunk_create's tail slack (mrp_pack_kernel reads a read's last
 * bytes a dword at a time) and 256-byte alignment. */
int ScRun::layout_and_items(double het_substitution_probability) {
    lay.resize((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) { sc_layout(chunks[c], het_substitution_probability, lay[(size_t) c]); });
    dpool_base.assign((size_t) n_chunks + 1, 0);
    aoff_base.assign((size_t) n_chunks + 1, 0);
    seq_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        dpool_base[(size_t) c + 1] = (dpool_base[(size_t) c] + lay[(size_t) c].pool_bytes + MRP_POOL_TAIL_PAD + 255) & ~(int64_t) 255;
        aoff_base[(size_t) c + 1] = aoff_base[(size_t) c] + chunks[c].n_bubbles + 1;
        seq_base[(size_t) c + 1] = seq_base[(size_t) c] + (int64_t) lay[(size_t) c].seqs.size();
    }
    dpool_bytes = dpool_base[(size_t) n_chunks];
    n_seqs_all = seq_base[(size_t) n_chunks];
    items.resize((size_t) n_subs);
    aoff_all.resize((size_t) aoff_base[(size_t) n_chunks]);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_string_chunk &S = chunks[c];
        const ScLayout &Lc = lay[(size_t) c];
        const int64_t sb = F->sub_base[(size_t) c];
        for (int64_t b = 0; b < S.n_bubbles; b++)
            for (int64_t k = S.sub_first[b]; k < S.sub_first[b + 1]; k++) {
                const mrp_read &q = Lc.seqs[(size_t) Lc.seq_of[(size_t) S.sub_read[k]]];
                ScByteItem &it = items[(size_t) (sb + k)];
                it.dst = dpool_base[(size_t) c] + q.pool_offset + (Lc.aoff[(size_t) b] - Lc.aoff[(size_t) q.ref_start]);
                it.pair = (int32_t) F->pair_first[(size_t) (sb + k)];
                it.n_alleles = (int32_t) Lc.an[(size_t) b];
            }
        std::copy(Lc.aoff.begin(), Lc.aoff.end(), aoff_all.begin() + aoff_base[(size_t) c]);
    });
    return MRP_OK;
}

/* the profile bytes, written into the chunks' device pool; the host copy comes back behind them (EV_POOL_HOME) */
int ScRun::profile_bytes() {
    PHM_HIP(d_items.upload(items, s));
    PHM_HIP(d_aoff.upload(aoff_all, s));
    const int rc = back.upload_static(*this); /* the static tables of the back half go up with the rest */
    if (rc != MRP_OK) return rc;
    PHM_HIP(d_pool.alloc((size_t) dpool_bytes));
    PHM_HIP(hipMemsetAsync(d_pool.p, 0, (size_t) dpool_bytes, s)); /* sites a read skips stay 0 */
    PHM_HIP(h_pool.reserve((size_t) dpool_bytes));
    PHM_HIP(hipEventRecord(ev[EV_BYTES_BEGIN], s));
    if (n_subs > 0) {
        hipLaunchKernelGGL(sc_profile_bytes_kernel, dim3((unsigned) ((n_subs + 255) / 256)), dim3(256), 0, s, d_items.p, n_subs, D.d_out.p, d_pool.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ev[EV_BYTES_END], s));
    PHM_HIP(hipMemcpyAsync(h_pool.p, d_pool.p, (size_t) dpool_bytes, hipMemcpyDeviceToHost, s));
    PHM_HIP(hipEventRecord(ev[EV_POOL_HOME], s)); /* the host copy is complete */
    return MRP_OK;
}

/* chunks over that pool (site tables staged and uploaded behind the download), then the phasing as it stands */
int ScRun::chunks_and_phase(const mrp_params *params) {
    std::vector<mrp_chunk_desc> descs((size_t) n_chunks);
    std::vector<const mrp_chunk_desc *> desc_ptr((size_t) n_chunks);
    std::vector<const uint8_t *> dev_pools((size_t) n_chunks);
    std::vector<const mrp_read *> rptr((size_t) n_chunks);
    std::vector<int64_t> nr((size_t) n_chunks);
    for (int64_t c = 0; c < n_chunks; c++) {
        const ScLayout &Lc = lay[(size_t) c];
        mrp_chunk_desc &d = descs[(size_t) c];
        d.n_sites = chunks[c].n_bubbles;
        d.allele_number = Lc.an.data();
        d.substitution_log_probs = Lc.sub.data();
        d.allele_prior_log_probs = Lc.prior.data();
        d.profile_pool = (const uint8_t *) h_pool.p + dpool_base[(size_t) c];
        d.pool_bytes = Lc.pool_bytes;
        d.reads = Lc.seqs.data();
        d.n_reads = (int64_t) Lc.seqs.size();
        desc_ptr[(size_t) c] = &d;
        dev_pools[(size_t) c] = d_pool.p + dpool_base[(size_t) c];
        rptr[(size_t) c] = Lc.seqs.data();
        nr[(size_t) c] = (int64_t) Lc.seqs.size();
    }
    int rc = mrp_chunk_block_create(ctx, n_chunks, desc_ptr.data(), dch.data(), &blk, 1, dev_pools.data());
    if (rc != MRP_OK) return rc;
    for (mrp_chunk *ch : dch) { ch->pool_host_ready = ev[EV_POOL_HOME]; ch->pool_host_pending.store(true); }
    std::vector<const mrp_chunk *> cptr(dch.begin(), dch.end());
    const double t0 = now_ms();
    rc = mrp_phase_reads_many(ctx, n_chunks, cptr.data(), rptr.data(), nr.data(), params, res.data(), stats ? &stats->phase : nullptr);
    phase_ms = now_ms() - t0;
    return rc;
}

/* HP tags over the same device pool: the fragments' haplotype strings go up, one lane per sequence; the back half follows the HP
 * kernel on the same stream and reads the tags and the haplotype strings where they are */
int ScRun::hp_tags(int64_t min_phred) {
    hap_base.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) hap_base[(size_t) c + 1] = hap_base[(size_t) c] + 2 * (int64_t) res[(size_t) c]->length;
    haps.resize((size_t) hap_base[(size_t) n_chunks]);
    hitems.resize((size_t) n_seqs_all);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_phase_result *g = res[(size_t) c];
        const ScLayout &Lc = lay[(size_t) c];
        const int64_t ns = (int64_t) Lc.seqs.size();
        if (g->length > 0) {
            std::copy(g->haplotype_string1, g->haplotype_string1 + g->length, haps.begin() + hap_base[(size_t) c]);
            std::copy(g->haplotype_string2, g->haplotype_string2 + g->length, haps.begin() + hap_base[(size_t) c] + g->length);
        }
        std::vector<int32_t> side((size_t) ns, 0);
        for (int64_t q = 0; q < g->n_reads2; q++) /* a read found in both sets counts as hap1 (genomeFragment.c:253) */
            if (g->reads2[q] >= 0 && g->reads2[q] < ns) side[(size_t) g->reads2[q]] = 2;
        for (int64_t q = 0; q < g->n_reads1; q++)
            if (g->reads1[q] >= 0 && g->reads1[q] < ns) side[(size_t) g->reads1[q]] = 1;
        for (int64_t q = 0; q < ns; q++) {
            ScHapItem &it = hitems[(size_t) (seq_base[(size_t) c] + q)];
            it.pool = dpool_base[(size_t) c] + Lc.seqs[(size_t) q].pool_offset;
            it.aoff = aoff_base[(size_t) c];
            it.hap = hap_base[(size_t) c];
            it.ref_start = Lc.seqs[(size_t) q].ref_start;
            it.length = Lc.seqs[(size_t) q].length;
            it.frag_start = g->ref_start;
            it.frag_length = g->length;
            it.side = side[(size_t) q];
            it.pad = 0;
        }
    }
    PHM_HIP(d_haps.upload(haps, s));
    PHM_HIP(d_hitems.upload(hitems, s));
    PHM_HIP(d_hap.alloc((size_t) n_seqs_all));
    PHM_HIP(d_phred.alloc((size_t) n_seqs_all));
    PHM_HIP(h_res.reserve((size_t) n_seqs_all * 9 + 16));
    h_hap = (int8_t *) h_res.p;
    h_phred = (double *) ((char *) h_res.p + (((size_t) n_seqs_all + 7) & ~(size_t) 7));
    /* the back half's buffers, device and pinned, before the HP kernel is queued: no allocation between it and the back half */
    int rc = back.alloc_results(*this);
    if (rc != MRP_OK) return rc;
    PHM_HIP(hipEventRecord(ev[EV_TAGS_BEGIN], s));
    if (n_seqs_all > 0) {
        hipLaunchKernelGGL(sc_assign_kernel, dim3((unsigned) ((n_seqs_all + 255) / 256)), dim3(256), 0, s, d_hitems.p, n_seqs_all, d_aoff.p, d_haps.p,
                           d_pool.p, min_phred, d_hap.p, d_phred.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ctx->ev[1], s));
    if (n_seqs_all > 0) {
        PHM_HIP(hipMemcpyAsync(h_hap, d_hap.p, (size_t) n_seqs_all, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h_phred, d_phred.p, (size_t) n_seqs_all * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    return back.launch(*this);
}

/* the downloads queued behind their kernels have landed once the stream has drained */
int ScRun::download() {
    PHM_HIP(hipStreamSynchronize(s));
    /* (read before anything is handed over: an error leaves profiles_out / filtered_out zeroed) */
    if (back.on && filtered_stats) PHM_HIP(hipEventElapsedTime(&back.ms, ev[EV_BACK_BEGIN], ev[EV_BACK_END]));
    return MRP_OK;
}

/* back to the caller's reads; the results are the caller's from the last line on */
int ScRun::hand_over(mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out) {
    for (int64_t c = 0; c < n_chunks; c++) {
        const ScLayout &Lc = lay[(size_t) c];
        mrp_phase_result *g = res[(size_t) c];
        for (int64_t r = 0; r < chunks[c].n_reads; r++) {
            hap_out[c][r] = -1;
            if (phred_out) phred_out[c][r] = 0.0;
        }
        for (size_t q = 0; q < Lc.seqs.size(); q++) {
            const int32_t r = Lc.read_of_seq[q];
            hap_out[c][r] = h_hap[seq_base[(size_t) c] + (int64_t) q];
            if (phred_out) phred_out[c][r] = h_phred[seq_base[(size_t) c] + (int64_t) q];
        }
        for (int64_t q = 0; q < g->n_reads1; q++) g->reads1[q] = Lc.read_of_seq[(size_t) g->reads1[q]];
        for (int64_t q = 0; q < g->n_reads2; q++) g->reads2[q] = Lc.read_of_seq[(size_t) g->reads2[q]];
    }
    if (profiles_out)
        for (int64_t c = 0; c < n_chunks; c++) {
            const ScLayout &Lc = lay[(size_t) c];
            mrp_profile_out &P = profiles_out[c];
            P.n_seqs = (int64_t) Lc.seqs.size();
            P.pool_bytes = Lc.pool_bytes;
            P.seqs = (mrp_read *) sc_dup(Lc.seqs.data(), sizeof(mrp_read) * Lc.seqs.size());
            P.read_of_seq = (int32_t *) sc_dup(Lc.read_of_seq.data(), sizeof(int32_t) * Lc.read_of_seq.size());
            P.pool = (uint8_t *) sc_dup((const uint8_t *) h_pool.p + dpool_base[(size_t) c], (size_t) Lc.pool_bytes);
            P.allele_number = (uint32_t *) sc_dup(Lc.an.data(), sizeof(uint32_t) * Lc.an.size());
            P.substitution = (uint16_t *) sc_dup(Lc.sub.data(), sizeof(uint16_t) * Lc.sub.size());
            P.prior = (uint16_t *) sc_dup(Lc.prior.data(), sizeof(uint16_t) * Lc.prior.size());
            if (!P.seqs || !P.read_of_seq || !P.pool || !P.allele_number || !P.substitution || !P.prior) {
                for (int64_t q = 0; q <= c; q++) mrp_profile_out_clear(&profiles_out[q]);
                return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks: out of host memory");
            }
        }
    const int rc = back.hand_over(*this, profiles_out);
    if (rc != MRP_OK) return rc;
    if (stats) {
        float ms = 0.f;
        if (n_pairs > 0) { PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ev[EV_PAIRS_END])); stats->pairhmm.kernel_ms = ms; stats->pairhmm.cells = F->L.cells; }
        PHM_HIP(hipEventElapsedTime(&ms, ev[EV_BYTES_BEGIN], ev[EV_BYTES_END]));
        stats->profile_ms = ms;
        PHM_HIP(hipEventElapsedTime(&ms, ev[EV_TAGS_BEGIN], ctx->ev[1]));
        stats->assign_ms = ms;
    }
    for (int64_t c = 0; c < n_chunks; c++) { out[c] = res[(size_t) c]; res[(size_t) c] = nullptr; }
    return MRP_OK;
}

/* the static tables; a read's tag is its sequence's (read_seq: -1 a primary read in no bubble, -2 a filtered read) */
int ScRun::Back::upload_static(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    n_reads = Q.read_base[(size_t) R.n_chunks];
    n_vars = Q.var_base[(size_t) R.n_chunks];
    n_tot = 2 * (size_t) (n_reads + n_vars);
    n_i32 = (size_t) (n_reads + n_vars);
    read_seq.resize((size_t) n_reads);
    for (int64_t c = 0; c < R.n_chunks; c++) {
        const int64_t rb = Q.read_base[(size_t) c];
        for (int64_t r = 0; r < R.chunks[c].n_reads; r++) {
            const int32_t q = R.lay[(size_t) c].seq_of[(size_t) r];
            read_seq[(size_t) (rb + r)] = q < 0 ? -1 : (int32_t) (R.seq_base[(size_t) c] + q);
        }
        for (int64_t r = 0; r < Q.rest[c].n_filtered; r++) read_seq[(size_t) (rb + R.chunks[c].n_reads + r)] = -2;
    }
    PHM_HIP(d_ent.upload(Q.entries, s));
    PHM_HIP(d_sites.upload(Q.sites, s));
    PHM_HIP(d_cbase.upload(Q.cbase, s));
    PHM_HIP(d_pidx.upload(Q.pidx, s));
    PHM_HIP(d_cand_first.upload(Q.cand_first, s));
    PHM_HIP(d_cand.upload(Q.cand, s));
    PHM_HIP(d_read_seq.upload(read_seq, s));
    return MRP_OK;
}

/* what the phasing decided per chunk goes up; then every buffer of the results.  Totals: h1 | h2 of the reads, then cis | trans of
 * the variants; decisions: the reads', then the variants'. */
int ScRun::Back::alloc_results(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    fchunks.resize((size_t) R.n_chunks);
    for (int64_t c = 0; c < R.n_chunks; c++)
        fchunks[(size_t) c] = FsChunk{R.hap_base[(size_t) c], (int32_t) R.res[(size_t) c]->ref_start, (int32_t) R.res[(size_t) c]->length};
    PHM_HIP(d_chunks.upload(fchunks, s));
    PHM_HIP(d_rec.alloc(Q.entries.size()));
    PHM_HIP(d_tot.alloc(n_tot));
    PHM_HIP(d_hap.alloc(n_i32));
    PHM_HIP(h_res.reserve(n_tot * sizeof(double) + n_i32 * sizeof(int32_t) + (count_used ? (size_t) R.n_pairs : 0) + 16));
    h_tot = (double *) h_res.p;
    h_hap = (int32_t *) (h_tot + n_tot);
    h_used = (uint8_t *) (h_hap + n_i32);
    if (count_used) {
        PHM_HIP(d_used.alloc((size_t) R.n_pairs));
        PHM_HIP(hipMemsetAsync(d_used.p, 0, (size_t) std::max<int64_t>(R.n_pairs, 1), s));
    }
    return MRP_OK;
}

int ScRun::Back::launch(ScRun &R) {
    if (!on) return MRP_OK;
    hipStream_t s = R.s;
    const int64_t n_sites = (int64_t) Q.sites.size();
    PHM_HIP(hipEventRecord(R.ev[EV_BACK_BEGIN], s));
    if (n_sites > 0) {
        hipLaunchKernelGGL(sc_filtered_sites_kernel, dim3((unsigned) n_sites), dim3(64), 0, s, d_sites.p, d_ent.p, d_cbase.p, d_pidx.p, d_read_seq.p,
                           R.d_hap.p, d_chunks.p, R.d_haps.p, d_rec.p, count_used ? d_used.p : nullptr);
        PHM_HIP(hipGetLastError());
    }
    double *d_h1 = d_tot.p, *d_h2 = d_tot.p + n_reads, *d_cis = d_tot.p + 2 * n_reads, *d_trans = d_cis + n_vars;
    if (n_reads > 0) {
        hipLaunchKernelGGL(fs_partition_kernel, dim3((unsigned) ((n_reads + 255) / 256)), dim3(256), 0, s, d_cand_first.p, d_cand.p, d_rec.p, R.D.d_out.p,
                           d_read_seq.p, R.d_hap.p, n_reads, d_hap.p, d_h1, d_h2);
        PHM_HIP(hipGetLastError());
    }
    if (n_vars > 0) {
        hipLaunchKernelGGL(fs_phase_kernel, dim3((unsigned) ((n_vars + 255) / 256)), dim3(256), 0, s, d_sites.p + Q.n_bsites, d_rec.p, R.D.d_out.p, n_vars,
                           d_hap.p + n_reads, d_cis, d_trans);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(R.ev[EV_BACK_END], s));
    if (n_tot > 0) {
        PHM_HIP(hipMemcpyAsync(h_tot, d_tot.p, n_tot * sizeof(double), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h_hap, d_hap.p, n_i32 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (count_used && R.n_pairs > 0) PHM_HIP(hipMemcpyAsync(h_used, d_used.p, (size_t) R.n_pairs, hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

int ScRun::Back::hand_over(ScRun &R, mrp_profile_out *profiles_out) {
    if (!on) return MRP_OK;
    const double *h_h1 = h_tot, *h_h2 = h_tot + n_reads, *h_cis = h_tot + 2 * n_reads, *h_trans = h_cis + n_vars;
    bool ok = true;
    for (int64_t c = 0; c < R.n_chunks && ok; c++) {
        mrp_filtered_out &O = out[c];
        const int64_t rb = Q.read_base[(size_t) c], nr = Q.read_base[(size_t) c + 1] - rb, vb = Q.var_base[(size_t) c], nv = Q.var_base[(size_t) c + 1] - vb;
        O.n_reads = nr;
        O.n_variants = nv;
        O.read_hap = (int32_t *) sc_dup(h_hap + rb, sizeof(int32_t) * (size_t) nr);
        O.h1 = (double *) sc_dup(h_h1 + rb, sizeof(double) * (size_t) nr);
        O.h2 = (double *) sc_dup(h_h2 + rb, sizeof(double) * (size_t) nr);
        O.variant_state = (int32_t *) sc_dup(h_hap + n_reads + vb, sizeof(int32_t) * (size_t) nv);
        O.cis = (double *) sc_dup(h_cis + vb, sizeof(double) * (size_t) nv);
        O.trans = (double *) sc_dup(h_trans + vb, sizeof(double) * (size_t) nv);
        ok = O.read_hap && O.h1 && O.h2 && O.variant_state && O.cis && O.trans;
    }
    if (!ok) {
        for (int64_t c = 0; c < R.n_chunks; c++) {
            mrp_filtered_out_clear(&out[c]);
            if (profiles_out) mrp_profile_out_clear(&profiles_out[c]);
        }
        return fail(MRP_ERR_NOMEM, "mrp_phase_string_chunks_with_filtered: out of host memory");
    }
    if (R.filtered_stats) {
        mrp_string_filtered_stats &T = *R.filtered_stats;
        T.filtered_ms += ms;
        T.pairs_scored += R.n_pairs;
        T.pairs_speculative += R.n_pairs - Q.n_primary_pairs;
        for (int64_t p = Q.n_primary_pairs; p < R.n_pairs; p++) T.pairs_read_by_results += h_used[p] ? 1 : 0;
    }
    return MRP_OK;
}

}  // namespace

int mrp_string_front_run(mrp_context *ctx, mrp_string_front *F, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                         mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                         mrp_string_chunks_stats *stats, mrp_filtered_out *filtered_out, mrp_string_filtered_stats *filtered_stats) {
    const double t_begin = now_ms();
    int rc;
    double phase_ms;
    {
        ScRun R(ctx, F, stats, filtered_out, filtered_stats);
        rc = R.begin();
        if (rc == MRP_OK) rc = R.enqueue_pairhmm();
        if (rc == MRP_OK) rc = R.layout_and_items(het_substitution_probability);
        if (rc == MRP_OK) rc = R.profile_bytes();
        if (rc == MRP_OK) rc = R.chunks_and_phase(params);
        if (rc == MRP_OK) rc = R.hp_tags(min_phred);
        if (rc == MRP_OK) rc = R.download();
        if (rc == MRP_OK) rc = R.hand_over(out, hap_out, phred_out, profiles_out);
        phase_ms = R.phase_ms;
    }
    /* the stream has drained and every buffer of the run is back in the pool (after a refused run as well) */
    ctx->pool.reclaim();
    if (rc == MRP_OK && stats) { /* the whole call, its teardown included */
        stats->total_ms = F->front_ms + (now_ms() - t_begin);
        stats->host_ms = stats->total_ms - phase_ms;
    }
    return rc;
}

extern "C" {

int mrp_string_chunk_units(const mrp_string_chunk *chunk, int64_t *units_out) {
    if (!chunk || !units_out || chunk->n_bubbles < 0 || (chunk->n_bubbles > 0 && !chunk->sub_first))
        return mrp_set_error(MRP_ERR_ARG, "mrp_string_chunk_units: null argument or bad sizes");
    *units_out = chunk->n_bubbles ? chunk->sub_first[chunk->n_bubbles] : 0;
    return MRP_OK;
}

int mrp_phase_string_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model,
                            const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                            const mrp_params *params, int64_t min_phred, mrp_phase_result **out, int8_t *const *hap_out,
                            double *const *phred_out, mrp_profile_out *profiles_out, mrp_string_chunks_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    /* ---- checks (host only, before the context: a malformed call is refused the same with or without a device) */
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, nullptr, "mrp_phase_string_chunks");
    if (rc != MRP_OK) return rc;
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_phase_string_chunks: no context (the pair-HMM path has no CPU fallback)");
    for (int64_t c = 0; c < n_chunks; c++) out[c] = nullptr;
    if (profiles_out) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    if (n_chunks == 0) return MRP_OK;
    mrp_string_front *F = nullptr;
    rc = mrp_string_front_create(n_chunks, chunks, nullptr, forward_model, reverse_model, expansion, sv_threshold, &F);
    if (rc != MRP_OK) return rc;
    F->front_ms = now_ms() - t_begin;
    rc = mrp_string_front_run(ctx, F, het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, stats, nullptr, nullptr);
    mrp_string_front_destroy(F);
    return rc;
}

int mrp_phase_string_chunks_with_filtered(mrp_context *ctx, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest,
                                          const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                          double het_substitution_probability, const mrp_params *params, int64_t min_phred, mrp_phase_result **out,
                                          int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out, mrp_filtered_out *filtered_out,
                                          mrp_string_filtered_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks > 0 && (!rest || !filtered_out)) return fail(MRP_ERR_ARG, "mrp_phase_string_chunks_with_filtered: null argument or bad sizes");
    if (filtered_out && n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, rest, "mrp_phase_string_chunks_with_filtered");
    if (rc != MRP_OK) return rc;
    if (!ctx) return fail(MRP_ERR_NO_DEVICE, "mrp_phase_string_chunks_with_filtered: no context (the pair-HMM path has no CPU fallback)");
    for (int64_t c = 0; c < n_chunks; c++) out[c] = nullptr;
    if (profiles_out) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    if (n_chunks == 0) return MRP_OK;
    mrp_string_front *F = nullptr;
    rc = mrp_string_front_create(n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold, &F);
    if (rc != MRP_OK) return rc;
    F->front_ms = now_ms() - t_begin;
    rc = mrp_string_front_run(ctx, F, het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, stats ? &stats->chunks : nullptr,
                              filtered_out, stats);
    mrp_string_front_destroy(F);
    return rc;
}

}  // extern "C"

/* ---- mrp_haplotag_aligned_chunks: the staged extraction (mrp_internal.h) with the partition of mrp_partition_reads_by_haplotype reading
 * its result where it lies in HBM.  One device pool holds the call's allele strings, then the substrings the
 * gather writes behind them; the owners of equal substrings are found there (ha_owners_kernel); the host gets per entry its read, length
 * and owner and per read its status, and makes from them what needs no symbol: the pair list (ht_build_pairs' order), the launch classes
 * (phm_classify reads offsets and lengths only for unanchored pairs) and the per-read entry lists of ht_partition_kernel. */
namespace {

/* What the composites over aligned chunks share (mrp_haplotag_aligned_chunks, mrp_phase_aligned_chunks): the staged extraction gathering
 * behind the allele strings in the call's one device pool, the owners kernel over it and what comes back from it -- indices, no symbol. */
struct AlignedFront {
    const char *const who;
    mrp_context *const ctx;
    const int64_t n_chunks;
    const mrp_aligned_chunk *const chunks;
    mrp_extract_run *X = nullptr;
    hipStream_t s = nullptr; /* set once the device is current: from then on the destructor drains it */
    hipEvent_t ev[2] = {nullptr, nullptr}; /* around the owners kernel */
    mrp_extract_device D{};
    int64_t allele_bytes = 0, pool_bytes = 0, n_alleles = 0, downloaded = 0;
    PinnedBuf h_sym, h_back;
    HostVec<int64_t> a_off, y_off;
    HostVec<int32_t> a_len;
    HostVec<uint8_t> forward;
    DevBuf<uint8_t> d_sym, d_take;
    DevBuf<uint64_t> d_key;
    DevBuf<int32_t> d_owner;
    /* what came back after the owners kernel */
    const uint8_t *k_status = nullptr;
    const int64_t *k_first = nullptr, *k_len = nullptr;
    const int32_t *k_read = nullptr, *k_owner = nullptr;

    AlignedFront(const char *w, mrp_context *c, int64_t n, const mrp_aligned_chunk *ch) : who(w), ctx(c), n_chunks(n), chunks(ch) {}
    ~AlignedFront() {
        if (s) (void) hipStreamSynchronize(s);
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
        mrp_extract_run_destroy(X);
    }
    int extract();
    int owners(const HostVec<uint8_t> *take);
    void offsets_and_strands();
    void release() { d_sym.release(); d_take.release(); d_key.release(); d_owner.release(); }
};

struct HaRun : AlignedFront {
    const int32_t *const *const gt;
    mrp_haplotag_aligned_stats *const stats;
    PinnedBuf h_res;
    HostVec<int64_t> first;
    HostVec<HtEntry> ent;
    HtPairs P;
    PhmLaunch H;
    PhmDev L; /* L.d_out holds the log probabilities the partition kernel reads */
    DevBuf<int32_t> d_hap;
    DevBuf<int64_t> d_first;
    DevBuf<HtEntry> d_ent;
    DevBuf<double> d_h;

    HaRun(mrp_context *c, int64_t n, const mrp_aligned_chunk *ch, const int32_t *const *g, mrp_haplotag_aligned_stats *st)
        : AlignedFront("mrp_haplotag_aligned_chunks", c, n, ch), gt(g), stats(st) {}
    ~HaRun() {
        if (s) (void) hipStreamSynchronize(s); /* before the pinned result buffer goes */
    }
    int check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
              int8_t *const *hap_out, double *const *h1_out, double *const *h2_out);
    int pairs();
    int score(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion);
    int hand_over(int8_t *const *hap_out, double *const *h1_out, double *const *h2_out);
};

/* every MRP_ERR_ARG of the call, then the two refused modes: nothing here looks at the context */
int HaRun::check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                 int8_t *const *hap_out, double *const *h1_out, double *const *h2_out) {
    X = mrp_extract_run_create(who, n_chunks, chunks, options, stats ? &stats->extract : nullptr);
    if (!X) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int rc = mrp_extract_run_check_args(X, true);
    if (rc == MRP_OK) rc = mrp_extract_run_check_chunks(X);
    if (rc != MRP_OK) return rc;
    if (!forward_model || !reverse_model || (n_chunks > 0 && (!gt || !hap_out))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        if (C.n_reads > 0 && (!hap_out[c] || (h1_out && !h1_out[c]) || (h2_out && !h2_out[c])))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output array", who, (long long) c);
        if (C.n_variants > 0 && !gt[c]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null genotypes", who, (long long) c);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t k = C.allele_first[v + 1] - C.allele_first[v];
            for (int w = 0; w < 2; w++)
                if (gt[c][2 * v + w] < 0 || gt[c][2 * v + w] >= k)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, variant %lld: genotype %d outside its %lld alleles", who, (long long) c, (long long) v,
                                         gt[c][2 * v + w], (long long) k);
        }
    }
    return mrp_extract_run_check_modes(X);
}

/* the extraction up to its second half, gathering behind the allele strings in the call's one device pool */
int AlignedFront::extract() {
    int rc = mrp_extract_run_stage(X, ctx);
    if (rc != MRP_OK) return rc;
    s = ctx->stream;
    d_sym.pool = d_take.pool = d_key.pool = d_owner.pool = &ctx->pool;
    for (hipEvent_t &x : ev) PHM_HIP(hipEventCreate(&x));
    rc = mrp_extract_run_first_half(X);
    int64_t n_ent = 0, n_bases = 0;
    if (rc == MRP_OK) rc = mrp_extract_run_totals(X, &n_ent, &n_bases);
    if (rc != MRP_OK) return rc;
    downloaded += 16;
    allele_bytes = mrp_extract_run_allele_bytes(X);
    pool_bytes = allele_bytes + n_bases;
    for (int64_t c = 0; c < n_chunks; c++) n_alleles += chunks[c].n_variants ? chunks[c].allele_first[chunks[c].n_variants] : 0;
    a_off.resize((size_t) n_alleles);
    a_len.resize((size_t) n_alleles);
    PHM_HIP(h_sym.reserve(std::max<size_t>((size_t) allele_bytes, 1)));
    mrp_extract_run_alleles(X, (uint8_t *) h_sym.p, a_off.data(), a_len.data());
    PHM_HIP(d_sym.alloc((size_t) pool_bytes));
    if (allele_bytes) PHM_HIP(hipMemcpyAsync(d_sym.p, h_sym.p, (size_t) allele_bytes, hipMemcpyHostToDevice, s));
    rc = mrp_extract_run_second_half(X, d_sym.p, allele_bytes);
    if (rc != MRP_OK) return rc;
    mrp_extract_run_device(X, &D);
    return MRP_OK;
}

/* the owners on the device (take: NULL, or per read of the call whether it may take part); back come the per-read status and per entry
 * its read, length and owner -- not the symbols */
int AlignedFront::owners(const HostVec<uint8_t> *take) {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants, n_reads = D.n_reads;
    PHM_HIP(d_key.alloc((size_t) n_ent));
    PHM_HIP(d_owner.alloc((size_t) n_ent));
    if (take) PHM_HIP(d_take.upload(*take, s));
    PHM_HIP(hipEventRecord(ev[0], s));
    if (n_ent > 0) {
        hipLaunchKernelGGL(ha_owners_kernel, dim3((unsigned) std::min<int64_t>(n_var, 65536)), dim3(PHM_WAVE), 0, s, D.entry_first, n_var, D.entry_read,
                           D.read_status, D.entry_len, D.entry_off, D.symbols, take ? (const uint8_t *) d_take.p : nullptr, d_key.p, d_owner.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ev[1], s));
    const size_t b_first = 0, b_len = b_first + 8 * ((size_t) n_var + 1), b_read = b_len + 8 * (size_t) n_ent, b_owner = b_read + 4 * (size_t) n_ent,
                 b_status = b_owner + 4 * (size_t) n_ent, b_end = b_status + (size_t) n_reads;
    PHM_HIP(h_back.reserve(b_end));
    uint8_t *hk = (uint8_t *) h_back.p;
    PHM_HIP(hipMemcpyAsync(hk + b_first, D.entry_first, 8 * ((size_t) n_var + 1), hipMemcpyDeviceToHost, s));
    if (n_ent) {
        PHM_HIP(hipMemcpyAsync(hk + b_len, D.entry_len, 8 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(hk + b_read, D.entry_read, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(hk + b_owner, d_owner.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
    }
    if (n_reads) PHM_HIP(hipMemcpyAsync(hk + b_status, D.read_status, (size_t) n_reads, hipMemcpyDeviceToHost, s));
    PHM_HIP(hipStreamSynchronize(s));
    downloaded += (int64_t) b_end;
    k_first = (const int64_t *) (hk + b_first);
    k_len = (const int64_t *) (hk + b_len);
    k_read = (const int32_t *) (hk + b_read);
    k_owner = (const int32_t *) (hk + b_owner);
    k_status = hk + b_status;
    return MRP_OK;
}

/* where every entry's symbols lie in the device pool (behind the allele strings, in entry order), and every read's strand */
void AlignedFront::offsets_and_strands() {
    const int64_t n_ent = D.n_entries;
    y_off.resize((size_t) n_ent);
    int64_t at = allele_bytes;
    for (int64_t p = 0; p < n_ent; p++) { y_off[(size_t) p] = at; at += k_len[p]; }
    forward.resize((size_t) D.n_reads);
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) forward[(size_t) (D.read_first[c] + r)] = (chunks[c].flag[r] & 0x10) == 0;
}

/* on the host, from indices and lengths alone: the two pairs of every owner at an active site in ht_build_pairs' order (the model from
 * the owner's strand), and every read's entries in site order */
int HaRun::pairs() {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants, n_reads = D.n_reads;
    offsets_and_strands();
    std::vector<uint8_t> active((size_t) n_var, 0);
    P.pair_of.assign((size_t) n_ent, -1);
    first.assign((size_t) n_reads + 1, 0);
    int64_t n_active = 0, n_scored = 0, n_owners = 0, abase = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t g = D.variant_first[c] + v;
            if (gt[c][2 * v] == gt[c][2 * v + 1]) continue; /* bubbleGraph.c:1975 */
            int64_t k = 0;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++)
                if (k_owner[p] >= 0) { k++; first[(size_t) k_read[p] + 1]++; }
            if (!k) continue; /* :1989 */
            active[(size_t) g] = 1;
            n_active++;
            n_scored += k;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                if (k_owner[p] != p) continue;
                n_owners++;
                P.pair_of[(size_t) p] = P.list.size();
                for (int w = 0; w < 2; w++) { /* never anchored (:2027) */
                    const int64_t j = abase + C.allele_first[v] + gt[c][2 * v + w];
                    P.list.add(a_off[(size_t) j], a_len[(size_t) j], y_off[(size_t) p], (int32_t) k_len[p], forward[(size_t) k_read[p]] ? 0 : 1, nullptr);
                }
            }
        }
        abase += C.n_variants ? C.allele_first[C.n_variants] : 0;
    }
    for (int64_t r = 0; r < n_reads; r++) first[(size_t) r + 1] += first[(size_t) r];
    ent.resize((size_t) first[(size_t) n_reads]);
    std::vector<int64_t> fill(first.begin(), first.end() - 1);
    for (int64_t g = 0; g < n_var; g++) {
        if (!active[(size_t) g]) continue;
        for (int64_t p = k_first[g + 1] - 1; p >= k_first[g]; p--) { /* b->reads order (:2076) */
            if (k_owner[p] < 0) continue;
            const int64_t q = P.pair_of[(size_t) k_owner[p]];
            ent[(size_t) fill[(size_t) k_read[p]]++] = HtEntry{(int32_t) q, (int32_t) q + 1, 0, 0};
        }
    }
    if (stats) {
        stats->sites = n_var;
        stats->active_sites = n_active;
        stats->entries = n_scored;
        stats->owners = n_owners;
    }
    return MRP_OK;
}

/* the pair-HMM kernels over the pool that is already on the device, then a lane per read over its entries; the results on their way back */
int HaRun::score(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion) {
    const int64_t n_reads = D.n_reads;
    d_hap.pool = d_first.pool = d_ent.pool = d_h.pool = &ctx->pool;
    mrp_pairhmm_stats *pst = stats ? &stats->pairhmm : nullptr;
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    if (P.list.size() > 0) { /* (MRP_ERR_UNSUPPORTED for a diagonal beyond the limit is raised by phm_classify, before anything is launched) */
        int rc = phm_classify(who, models, 2, pool_bytes, P.list.view(), expansion, 0, 0, H);
        if (rc == MRP_OK) rc = phm_enqueue(ctx, nullptr, pool_bytes, P.list.size(), H, L, pst, d_sym.p);
        if (rc != MRP_OK) return rc;
    } else {
        if (stats) PHM_HIP(hipStreamSynchronize(s));
        PHM_HIP(hipEventRecord(ctx->ev[0], s));
    }
    PHM_HIP(d_first.upload(first, s));
    PHM_HIP(d_ent.upload(ent, s));
    PHM_HIP(d_hap.alloc((size_t) n_reads));
    PHM_HIP(d_h.alloc(2 * (size_t) n_reads));
    if (n_reads > 0) {
        hipLaunchKernelGGL(ht_partition_kernel, dim3((unsigned) ((n_reads + 255) / 256)), dim3(256), 0, s, d_first.p, d_ent.p, L.d_out.p, n_reads, d_hap.p, d_h.p,
                           d_h.p + n_reads);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ctx->ev[1], s));
    PHM_HIP(h_res.reserve(std::max<size_t>(20 * (size_t) n_reads, 1)));
    if (n_reads > 0) {
        PHM_HIP(hipMemcpyAsync(h_res.p, d_h.p, 16 * (size_t) n_reads, hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync((uint8_t *) h_res.p + 16 * (size_t) n_reads, d_hap.p, 4 * (size_t) n_reads, hipMemcpyDeviceToHost, s));
    }
    PHM_HIP(hipStreamSynchronize(s));
    downloaded += 20 * n_reads;
    return MRP_OK;
}

/* after the stream has drained: the outputs per chunk, the stats, the device arrays back to the pool */
int HaRun::hand_over(int8_t *const *hap_out, double *const *h1_out, double *const *h2_out) {
    const int64_t n_reads = D.n_reads;
    const double *k_h1 = (const double *) h_res.p, *k_h2 = k_h1 + n_reads;
    const int32_t *k_hap = (const int32_t *) (k_h2 + n_reads);
    if (stats) {
        float ms = 0.f;
        PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        stats->pairhmm.kernel_ms = ms;
        stats->pairhmm.cells = H.cells;
        PHM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stats->owners_ms = ms;
        stats->bytes_downloaded = downloaded;
        const int rc = mrp_extract_run_stats(X);
        if (rc != MRP_OK) return rc;
        mrp_extract_run_times(X, false);
    }
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) {
            const int64_t g = D.read_first[c] + r;
            const bool kept = k_status[g] == MRP_READ_KEPT;
            hap_out[c][r] = kept ? (int8_t) k_hap[g] : (int8_t) -1;
            if (h1_out) h1_out[c][r] = kept ? k_h1[g] : 0.0;
            if (h2_out) h2_out[c][r] = kept ? k_h2[g] : 0.0;
        }
    release();
    d_hap.release(); d_first.release(); d_ent.release(); d_h.release();
    L.d_models.release(); L.d_band.release(); L.d_out.release();
    for (int c = 0; c < 4; c++) { L.d_lane[c].release(); L.d_wave[c].release(); }
    mrp_extract_run_release(X); /* (reclaims the context's pool) */
    return MRP_OK;
}

}  // namespace

extern "C" int mrp_haplotag_aligned_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const int32_t *const *gt,
                                           const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                           int64_t expansion, int8_t *const *hap_out, double *const *h1_out, double *const *h2_out,
                                           mrp_haplotag_aligned_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    HaRun R(ctx, n_chunks, chunks, gt, stats);
    int rc = R.check(options, forward_model, reverse_model, expansion, hap_out, h1_out, h2_out);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction and the pair-HMM have no CPU fallback)", R.who);
    rc = R.extract();
    if (rc == MRP_OK) rc = R.owners(nullptr);
    if (rc == MRP_OK) rc = R.pairs();
    if (rc == MRP_OK) rc = R.score(forward_model, reverse_model, expansion);
    if (rc == MRP_OK) rc = R.hand_over(hap_out, h1_out, h2_out);
    if (rc != MRP_OK) return rc;
    if (stats) stats->total_ms = now_ms() - t_begin;
    return MRP_OK;
}

/* ---- mrp_phase_aligned_chunks: the staged extraction, the owners kernel with the caller's mask, the k-mer anchors on the device
 * (mrp_anchors.hip) and the string call's run over the pool where it lies in HBM.  The host makes, from indices
 * and lengths alone, what mrp_string_chunk_from_extracted and mrp_string_front_create make from the downloaded symbols: every chunk's
 * mrp_string_chunk index arrays (offsets into the device pool), the owners' pairs in the front's order, and which pairs are anchored. */
namespace {

struct PaRun : AlignedFront {
    const char *const *const *const read_names;
    const uint8_t *const *const keep;
    mrp_phase_aligned_stats *const stats;
    struct ChunkArrays { /* what the mrp_string_chunk of a chunk points into */
        std::vector<int64_t> a_first{0}, a_off, s_first{0}, s_off, bubble_variant;
        std::vector<int32_t> a_len, s_len, s_read;
        std::vector<uint8_t> forward;
    };
    std::vector<ChunkArrays> arr;
    std::vector<mrp_string_chunk> sc;
    std::vector<int64_t> anchored; /* the pairs with a string longer than sv_threshold, ascending */
    std::vector<int64_t *> bv_out; /* the copies of bubble_variant the caller gets */
    mrp_string_front F;
    int64_t n_bubbles = 0, n_used = 0, n_owners = 0, n_anchors = 0, n_anchor_runs = 0;
    double anchors_ms = 0;
    /* the chunks of the call: all of the extraction's chunk records, or (with the filtered back half, PfRun) their first half -- the
     * second half are the same reads over the rests' variants */
    const int64_t n_front;
    std::vector<int64_t> entry_of_sub; /* with the back half: substring of the call -> its entry */

    PaRun(mrp_context *c, int64_t n, const mrp_aligned_chunk *ch, const char *const *const *names, const uint8_t *const *k, mrp_phase_aligned_stats *st,
          const char *w = "mrp_phase_aligned_chunks", int64_t front = -1)
        : AlignedFront(w, c, n, ch), read_names(names), keep(k), stats(st), n_front(front < 0 ? n : front) {}
    ~PaRun() {
        for (int64_t *p : bv_out) free(p);
    }
    int check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
              const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out);
    int masked_owners();
    int strings_and_pairs(int64_t sv_threshold);
    int anchors();
    int classify(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion);
    int hand_over(int64_t **bubble_variant_out);
};

/* every MRP_ERR_ARG of the call (the extraction's, then the string call's parameter checks), then the two refused modes: nothing
 * here looks at the context */
int PaRun::check(const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                 const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out) {
    X = mrp_extract_run_create(who, n_chunks, chunks, options, stats ? &stats->extract : nullptr);
    if (!X) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int rc = mrp_extract_run_check_args(X, true);
    if (rc == MRP_OK) rc = mrp_extract_run_check_chunks(X);
    if (rc != MRP_OK) return rc;
    if (!forward_model || !reverse_model || !params || (n_chunks > 0 && (!out || !hap_out || !read_names)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    for (int64_t c = 0; c < n_front; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        if (C.n_reads == 0) continue;
        if (!hap_out[c] || (phred_out && !phred_out[c])) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null output", who, (long long) c);
        if (!read_names[c]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null read names", who, (long long) c);
        for (int64_t r = 0; r < C.n_reads; r++)
            if (!read_names[c][r]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %lld has no name", who, (long long) c, (long long) r);
    }
    return mrp_extract_run_check_modes(X);
}

/* the owners among the kept reads the caller's mask lets through (one byte per read of the call; no mask anywhere: none uploaded) */
int PaRun::masked_owners() {
    bool any = n_front < n_chunks; /* (the second half's records take no part in the front) */
    for (int64_t c = 0; keep && c < n_front; c++) any = any || (keep[c] && chunks[c].n_reads > 0);
    if (!any) return owners(nullptr);
    HostVec<uint8_t> take((size_t) D.n_reads);
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++) take[(size_t) (D.read_first[c] + r)] = c >= n_front ? 0 : (keep && keep[c] ? (keep[c][r] != 0) : 1);
    return owners(&take);
}

/* bubbleGraph_constructFromVCFAndBamChunkReadVcfEntrySubstrings (bubbleGraph.c:1338-1400) over the device pool: a variant with an entry
 * that takes part is a bubble, its substrings those entries in descending order (:1391-1393); then mrp_string_front_create's pair list:
 * chunk by chunk, bubble by bubble, the owners in listing order, an owner's pairs allele by allele, the owner's strand picking the model */
int PaRun::strings_and_pairs(int64_t sv_threshold) {
    offsets_and_strands();
    const int64_t n_chunks = n_front;
    const bool back = n_front < AlignedFront::n_chunks;
    arr.resize((size_t) n_chunks);
    sc.assign((size_t) n_chunks, mrp_string_chunk{});
    std::vector<int64_t> &sub_base = F.sub_base, &pair_first = F.pair_first;
    sub_base.assign((size_t) n_chunks + 1, 0);
    pair_first.clear();
    std::vector<int64_t> sub_of((size_t) D.n_entries, -1); /* entry -> its substring in the call */
    PhmPairList &pairs = F.scratch.pairs;
    int64_t abase = 0, n_subs = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        ChunkArrays &A = arr[(size_t) c];
        A.forward.assign(forward.begin() + D.read_first[c], forward.begin() + D.read_first[c + 1]);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const int64_t g = D.variant_first[c] + v;
            int64_t k = 0;
            for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) k += k_owner[p] >= 0;
            if (!k) continue; /* :1366-1371 nothing to phase with */
            const int64_t na = C.allele_first[v + 1] - C.allele_first[v];
            if (na > 65535) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: variant %lld has more than 65535 alleles", who, (long long) c, (long long) v);
            const int64_t a0 = (int64_t) A.a_off.size();
            for (int64_t a = C.allele_first[v]; a < C.allele_first[v + 1]; a++) {
                A.a_off.push_back(a_off[(size_t) (abase + a)]);
                A.a_len.push_back(a_len[(size_t) (abase + a)]);
            }
            for (int64_t p = k_first[g + 1] - 1; p >= k_first[g]; p--) {
                if (k_owner[p] < 0) continue;
                sub_of[(size_t) p] = n_subs++;
                if (back) { /* what the back half's static front reads: a substring's owner and its entry */
                    F.scratch.owner.push_back(sub_of[(size_t) k_owner[p]]);
                    entry_of_sub.push_back(p);
                }
                /* the pair of the substring's owner with the bubble's allele 0 (the owner is listed before its duplicates) */
                pair_first.push_back(k_owner[p] == p ? pairs.size() : pair_first[(size_t) sub_of[(size_t) k_owner[p]]]);
                A.s_off.push_back(y_off[(size_t) p]);
                A.s_len.push_back((int32_t) k_len[p]);
                A.s_read.push_back((int32_t) (k_read[p] - D.read_first[c]));
                if (k_owner[p] != p) continue;
                n_owners++;
                const int model = forward[(size_t) k_read[p]] ? 0 : 1;
                for (int64_t j = 0; j < na; j++) {
                    const int32_t al = A.a_len[(size_t) (a0 + j)];
                    if (k_len[p] > sv_threshold || al > sv_threshold) anchored.push_back(pairs.size()); /* bubbleGraph.c:1448-1451 */
                    pairs.add(A.a_off[(size_t) (a0 + j)], al, y_off[(size_t) p], (int32_t) k_len[p], model, nullptr);
                }
            }
            A.bubble_variant.push_back(v);
            A.a_first.push_back((int64_t) A.a_off.size());
            A.s_first.push_back((int64_t) A.s_off.size());
        }
        abase += C.n_variants ? C.allele_first[C.n_variants] : 0;
        sub_base[(size_t) c + 1] = n_subs;
        mrp_string_chunk &S = sc[(size_t) c];
        S.n_bubbles = (int64_t) A.bubble_variant.size();
        S.n_reads = C.n_reads;
        S.pool = nullptr; /* the symbols are in HBM */
        S.pool_bytes = pool_bytes;
        S.allele_first = A.a_first.data();
        S.allele_off = A.a_off.data();
        S.allele_len = A.a_len.data();
        S.sub_first = A.s_first.data();
        S.sub_off = A.s_off.data();
        S.sub_len = A.s_len.data();
        S.sub_read = A.s_read.data();
        S.read_names = read_names[c];
        S.read_forward_strand = A.forward.data();
        n_bubbles += S.n_bubbles;
    }
    n_used = n_subs;
    if (pairs.size() >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    F.n_chunks = n_chunks;
    F.chunks = sc.data();
    F.n_subs = n_subs;
    F.n_pairs = pairs.size();
    F.device_pool = d_sym.p;
    F.device_pool_bytes = pool_bytes;
    return MRP_OK;
}

/* getKmerAlignmentAnchors of the anchored pairs, in the device pool; run counts and the anchors (as diagonal runs) come back and join
 * the pair list */
int PaRun::anchors() {
    PhmPairList &pairs = F.scratch.pairs;
    const int64_t n = (int64_t) anchored.size();
    if (n == 0) return MRP_OK;
    std::vector<int64_t> xo((size_t) n), yo((size_t) n), off((size_t) n + 1, 0), anc;
    std::vector<int32_t> xl((size_t) n), yl((size_t) n);
    for (int64_t i = 0; i < n; i++) {
        const size_t q = (size_t) anchored[(size_t) i];
        xo[(size_t) i] = pairs.x_off[q]; xl[(size_t) i] = pairs.x_len[q]; yo[(size_t) i] = pairs.y_off[q]; yl[(size_t) i] = pairs.y_len[q];
    }
    int64_t bytes = 0;
    const int rc = mrp_kmer_anchors_on_device(ctx, who, d_sym.p, n, xo.data(), xl.data(), yo.data(), yl.data(), off.data(), anc, &anchors_ms, &bytes, &n_anchor_runs);
    if (rc != MRP_OK) return rc;
    downloaded += bytes;
    n_anchors = off[(size_t) n];
    for (int64_t i = 0; i < n; i++) pairs.anchor_off[(size_t) anchored[(size_t) i] + 1] = off[(size_t) i + 1] - off[(size_t) i];
    pairs.counts_to_offsets();
    pairs.anchors = std::move(anc);
    return MRP_OK;
}

/* the launch classes and the bands; raises the 2 048-cell refusal, before any pair-HMM kernel */
int PaRun::classify(const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion) {
    if (F.n_pairs == 0) return MRP_OK;
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    return phm_classify(who, models, 2, pool_bytes, F.scratch.pairs.view(), expansion, 0, 0, F.L);
}

/* after the string run has handed its results over: the bubbles' variants, the stats, the device arrays back to the pool */
int PaRun::hand_over(int64_t **bubble_variant_out) {
    if (stats) {
        float ms = 0.f;
        PHM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stats->owners_ms = ms;
        stats->anchors_ms = anchors_ms;
        stats->variants = D.n_variants;
        stats->bubbles = n_bubbles;
        stats->entries = D.n_entries;
        stats->entries_used = n_used;
        stats->owners = n_owners;
        stats->pairs = F.n_pairs;
        stats->pairs_anchored = (int64_t) anchored.size();
        stats->anchors = n_anchors;
        stats->anchor_runs = n_anchor_runs;
        stats->front_bytes_downloaded = downloaded;
        const int rc = mrp_extract_run_stats(X);
        if (rc != MRP_OK) return rc;
        mrp_extract_run_times(X, false);
    }
    if (bubble_variant_out)
        for (int64_t c = 0; c < n_front; c++) { bubble_variant_out[c] = bv_out[(size_t) c]; bv_out[(size_t) c] = nullptr; }
    release();
    mrp_extract_run_release(X); /* (reclaims the context's pool) */
    return MRP_OK;
}

}  // namespace

extern "C" int mrp_phase_aligned_chunks(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const char *const *const *read_names,
                                        const uint8_t *const *keep, const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                        const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                                        const mrp_params *params, int64_t min_phred, mrp_phase_result **out, int8_t *const *hap_out,
                                        double *const *phred_out, mrp_profile_out *profiles_out, int64_t **bubble_variant_out,
                                        mrp_phase_aligned_stats *stats) {
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    PaRun R(ctx, n_chunks, chunks, read_names, keep, stats);
    int rc = R.check(options, forward_model, reverse_model, expansion, params, out, hap_out, phred_out);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction and the pair-HMM have no CPU fallback)", R.who);
    rc = R.extract();
    if (rc == MRP_OK) rc = R.masked_owners();
    if (rc == MRP_OK) rc = R.strings_and_pairs(sv_threshold);
    if (rc == MRP_OK) rc = R.anchors();
    if (rc == MRP_OK) rc = R.classify(forward_model, reverse_model, expansion);
    if (rc != MRP_OK) return rc;
    if (bubble_variant_out) { /* (made before anything is handed over: an error returns nothing) */
        R.bv_out.assign((size_t) n_chunks, nullptr);
        for (int64_t c = 0; c < n_chunks; c++) {
            std::vector<int64_t> bv = R.arr[(size_t) c].bubble_variant;
            bv.push_back(-1); /* the end of the list: the caller has no other way to the bubble count */
            R.bv_out[(size_t) c] = (int64_t *) sc_dup(bv.data(), sizeof(int64_t) * bv.size());
            if (!R.bv_out[(size_t) c]) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", R.who);
        }
    }
    for (int64_t c = 0; c < n_chunks; c++) out[c] = nullptr;
    if (profiles_out && n_chunks > 0) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    if (n_chunks > 0) {
        /* the rest of the string call unchanged: pair-HMM over the device pool, layout beside it, profile bytes, phasing, HP tags */
        R.F.front_ms = now_ms() - t_begin;
        rc = mrp_string_front_run(ctx, &R.F, het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out,
                                  stats ? &stats->chunks : nullptr, nullptr, nullptr);
        if (rc != MRP_OK) return rc;
    }
    rc = R.hand_over(bubble_variant_out);
    if (rc != MRP_OK) return rc;
    if (stats) stats->total_ms = now_ms() - t_begin;
    return MRP_OK;
}

/* ---- mrp_phase_aligned_chunks_with_filtered: mrp_phase_aligned_chunks with the back half of the chunk loop.
 * One staged extraction runs over 2 * n_chunks chunk records: record c is chunk c, record n_chunks + c the same reads over the rest's
 * variants (extractReadSubstringsAtVariantPositions called the second time, phase.c:354-357).  Both gathers land behind both sets of
 * allele strings in the call's one device pool.  The front is PaRun's, over the first half; ec_classes_kernel runs over the sites of
 * both halves, and from its representatives, the statuses and the entry indices the host makes what mrp_string_chunk_rest_from_extracted
 * makes from downloaded symbols -- every chunk's rest as index arrays into the device pool -- and the back half's static front
 * (sc_filtered_front, its classes by id).  The anchored pairs of both halves go through the anchors kernel in one launch. */
namespace {

struct PfRun : PaRun {
    const int64_t n; /* chunks of the call */
    const mrp_aligned_chunk_rest *const rest;
    struct RestArrays { /* what the mrp_string_chunk_rest of a chunk points into */
        std::vector<uint8_t> forward;
        std::vector<int64_t> f_first{0}, f_off, va_first{0}, va_off, ve_first{0}, ve_off;
        std::vector<int32_t> f_len, f_read, va_len, gt, ve_read, ve_len, filtered_read;
    };
    std::vector<RestArrays> ra;
    std::vector<mrp_string_chunk_rest> rs;
    std::vector<int32_t *> fr_out; /* the copies of filtered_read the caller gets */
    hipEvent_t cev[2] = {nullptr, nullptr}; /* around the classes kernel */
    DevBuf<uint64_t> d_ckey;
    DevBuf<int32_t> d_rep;
    PinnedBuf h_rep;
    int64_t n_filtered_reads = 0;

    PfRun(mrp_context *c, int64_t n_, const mrp_aligned_chunk *records, const mrp_aligned_chunk_rest *r, const char *const *const *names,
          const uint8_t *const *k, mrp_phase_aligned_stats *st)
        : PaRun(c, 2 * n_, records, names, k, st, "mrp_phase_aligned_chunks_with_filtered", n_), n(n_), rest(r) {}
    ~PfRun() {
        if (s) (void) hipStreamSynchronize(s); /* before the pinned buffer goes */
        for (hipEvent_t x : cev)
            if (x) (void) hipEventDestroy(x);
        for (int32_t *p : fr_out) free(p);
    }
    int check_rest() const;
    int classes();
    int rests();
    int filtered_front(int64_t sv_threshold);
};

/* the rest's own MRP_ERR_ARG (its variants have passed the extraction's checks as the second half's records) */
int PfRun::check_rest() const {
    for (int64_t c = 0; c < n; c++) {
        const mrp_aligned_chunk_rest &R = rest[c];
        if (R.n_variants > 0 && !R.gt) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null genotypes of the rest", who, (long long) c);
        for (int64_t v = 0; v < R.n_variants; v++) {
            const int64_t k = R.allele_first[v + 1] - R.allele_first[v];
            for (int w = 0; w < 2; w++)
                if (R.gt[2 * v + w] < 0 || R.gt[2 * v + w] >= k)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, filtered variant %lld: genotype %d outside its %lld alleles", who, (long long) c,
                                         (long long) v, R.gt[2 * v + w], (long long) k);
        }
    }
    return MRP_OK;
}

/* the classes of equal substrings at the sites of both halves, queued behind the gather; 4 B per entry start on their way back (the
 * owners' wait covers them) */
int PfRun::classes() {
    const int64_t n_ent = D.n_entries, n_var = D.n_variants;
    d_ckey.pool = d_rep.pool = &ctx->pool;
    for (hipEvent_t &x : cev) PHM_HIP(hipEventCreate(&x));
    PHM_HIP(d_ckey.alloc((size_t) n_ent));
    PHM_HIP(d_rep.alloc((size_t) n_ent));
    PHM_HIP(h_rep.reserve(std::max<size_t>(4 * (size_t) n_ent, 1)));
    PHM_HIP(hipEventRecord(cev[0], s));
    if (n_ent > 0) {
        hipLaunchKernelGGL(ec_classes_kernel<int64_t>, dim3((unsigned) std::min<int64_t>(n_var, 65536)), dim3(PHM_WAVE), 0, s, D.entry_first, n_var, D.entry_len,
                           D.entry_off, D.symbols, d_ckey.p, d_rep.p);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(cev[1], s));
    if (n_ent > 0) PHM_HIP(hipMemcpyAsync(h_rep.p, d_rep.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
    downloaded += 4 * n_ent;
    return MRP_OK;
}

/* mrp_string_chunk_rest_from_extracted over what came back: statuses, entry indices, lengths and representatives (the rules and their
 * reference lines are in include/margin_rphmm.h); offsets are into the device pool */
int PfRun::rests() {
    const int32_t *k_rep = (const int32_t *) h_rep.p;
    mrp_string_front::Scratch &X = F.scratch;
    ra.resize((size_t) n);
    rs.assign((size_t) n, mrp_string_chunk_rest{});
    X.fsub_cls.resize((size_t) n);
    X.ventry_cls.resize((size_t) n);
    X.sub_cls.resize(entry_of_sub.size());
    for (size_t k = 0; k < entry_of_sub.size(); k++) X.sub_cls[k] = k_rep[entry_of_sub[k]];
    int64_t abase = 0;
    for (int64_t c = 0; c < n; c++) abase += chunks[c].n_variants ? chunks[c].allele_first[chunks[c].n_variants] : 0;
    for (int64_t c = 0; c < n; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        const mrp_aligned_chunk_rest &Rc = rest[c];
        RestArrays &A = ra[(size_t) c];
        const int64_t nr = C.n_reads, nv = Rc.n_variants, r1 = D.read_first[c], r2 = D.read_first[n + c];
        auto primary = [&](int64_t r) { return k_status[r1 + r] == MRP_READ_KEPT && (!keep || !keep[c] || keep[c][r]); };
        auto kind = [&](int64_t r) {
            if (k_status[r1 + r] == MRP_READ_FILTERED) return 0;
            if (k_status[r1 + r] == MRP_READ_KEPT) return primary(r) ? -1 : 1;
            return k_status[r2 + r] == MRP_READ_KEPT ? 2 : -1;
        };
        int64_t n_kind[3] = {0, 0, 0};
        for (int64_t r = 0; r < nr; r++) {
            const int k = kind(r);
            if (k >= 0) n_kind[k]++;
        }
        const int64_t nf = n_kind[0] + n_kind[1] + n_kind[2];
        n_filtered_reads += nf;
        if (nf == 0 && nv == 0) continue; /* the empty rest */
        std::vector<int32_t> findex((size_t) nr, -1);
        A.filtered_read.resize((size_t) nf);
        A.forward.resize((size_t) nf);
        int64_t at[3] = {0, n_kind[0], n_kind[0] + n_kind[1]};
        for (int64_t r = 0; r < nr; r++) {
            const int k = kind(r);
            if (k < 0) continue;
            findex[(size_t) r] = (int32_t) at[k]++;
            A.filtered_read[(size_t) findex[(size_t) r]] = (int32_t) r;
            A.forward[(size_t) findex[(size_t) r]] = forward[(size_t) (r1 + r)];
        }
        std::vector<int64_t> &fcls = X.fsub_cls[(size_t) c], &vcls = X.ventry_cls[(size_t) c];
        for (int64_t v : arr[(size_t) c].bubble_variant) {
            const int64_t g = D.variant_first[c] + v;
            for (int pass = 0; pass < 2; pass++)
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                    const int64_t r = k_read[p] - r1;
                    if (kind(r) != pass) continue;
                    A.f_off.push_back(y_off[(size_t) p]);
                    A.f_len.push_back((int32_t) k_len[p]);
                    A.f_read.push_back(findex[(size_t) r]);
                    fcls.push_back(k_rep[p]);
                }
            A.f_first.push_back((int64_t) A.f_off.size());
        }
        for (int64_t v = 0; v < nv; v++) {
            const int64_t g = D.variant_first[n + c] + v;
            for (int64_t a = Rc.allele_first[v]; a < Rc.allele_first[v + 1]; a++) {
                A.va_off.push_back(a_off[(size_t) (abase + a)]);
                A.va_len.push_back(a_len[(size_t) (abase + a)]);
            }
            A.va_first.push_back((int64_t) A.va_off.size());
            A.gt.push_back(Rc.gt[2 * v]);
            A.gt.push_back(Rc.gt[2 * v + 1]);
            if (Rc.variant_pos[v] >= C.chunk_start && Rc.variant_pos[v] < C.chunk_end) /* bubbleGraph.c:2179 */
                for (int64_t p = k_first[g]; p < k_first[g + 1]; p++) {
                    const int64_t r = k_read[p] - r2;
                    if (k_status[r2 + r] != MRP_READ_KEPT) continue;
                    A.ve_read.push_back(primary(r) ? (int32_t) r : (int32_t) (nr + findex[(size_t) r]));
                    A.ve_off.push_back(y_off[(size_t) p]);
                    A.ve_len.push_back((int32_t) k_len[p]);
                    vcls.push_back(k_rep[p]);
                }
            A.ve_first.push_back((int64_t) A.ve_off.size());
        }
        abase += nv ? Rc.allele_first[nv] : 0;
        mrp_string_chunk_rest &R = rs[(size_t) c];
        R.n_filtered = nf;
        R.forward_strand = A.forward.data();
        R.pool = nullptr; /* the symbols are in HBM */
        R.pool_bytes = pool_bytes;
        R.fsub_first = A.f_first.data();
        R.fsub_off = A.f_off.data();
        R.fsub_len = A.f_len.data();
        R.fsub_read = A.f_read.data();
        R.n_variants = nv;
        R.valle_first = A.va_first.data();
        R.valle_off = A.va_off.data();
        R.valle_len = A.va_len.data();
        R.gt = A.gt.data();
        R.ventry_first = A.ve_first.data();
        R.ventry_read = A.ve_read.data();
        R.ventry_off = A.ve_off.data();
        R.ventry_len = A.ve_len.data();
    }
    return MRP_OK;
}

/* the back half's static front from indices and classes alone; its pairs past sv_threshold join the front's anchored list */
int PfRun::filtered_front(int64_t sv_threshold) {
    F.pool_base.assign((size_t) n + 1, 0); /* every offset is the device pool's already */
    F.scratch.classes_by_id = true;
    const std::vector<int64_t> rpool_base((size_t) n, 0);
    const int rc = sc_filtered_front(&F, rs.data(), sv_threshold, rpool_base);
    if (rc != MRP_OK) return rc;
    anchored.insert(anchored.end(), F.scratch.anchored_new.begin(), F.scratch.anchored_new.end());
    return MRP_OK;
}

}  // namespace

extern "C" int mrp_phase_aligned_chunks_with_filtered(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                      const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                      const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                      int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                      mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                                      int64_t **bubble_variant_out, mrp_filtered_out *filtered_out, int32_t **filtered_read_out,
                                                      mrp_phase_aligned_filtered_stats *stats) {
    static const char *who = "mrp_phase_aligned_chunks_with_filtered";
    const double t_begin = now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks < 0 || n_chunks >= (1ll << 30) || (n_chunks > 0 && (!chunks || !rest || !filtered_out || !filtered_read_out)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    /* the extraction's chunk records: the chunks, then the same reads over the rests' variants */
    std::vector<mrp_aligned_chunk> records((size_t) (2 * n_chunks));
    for (int64_t c = 0; c < n_chunks; c++) {
        records[(size_t) c] = chunks[c];
        mrp_aligned_chunk &R = records[(size_t) (n_chunks + c)];
        R = chunks[c];
        R.n_variants = rest[c].n_variants;
        R.variant_pos = rest[c].variant_pos;
        R.allele_first = rest[c].allele_first;
        R.allele_off = rest[c].allele_off;
        R.allele_len = rest[c].allele_len;
        R.allele_chars = rest[c].allele_chars;
        R.allele_bytes = rest[c].allele_bytes;
        R.is_sv = rest[c].is_sv;
    }
    PfRun R(ctx, n_chunks, records.data(), rest, read_names, keep, stats ? &stats->aligned : nullptr);
    int rc = R.check(options, forward_model, reverse_model, expansion, params, out, hap_out, phred_out);
    if (rc == MRP_OK || rc == MRP_ERR_UNSUPPORTED) { /* (every MRP_ERR_ARG comes before the refused modes) */
        const int rc2 = R.check_rest();
        if (rc2 != MRP_OK) rc = rc2;
    }
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction and the pair-HMM have no CPU fallback)", who);
    rc = R.extract();
    if (rc == MRP_OK) rc = R.classes();
    if (rc == MRP_OK) rc = R.masked_owners();
    if (rc == MRP_OK) rc = R.strings_and_pairs(sv_threshold);
    if (rc == MRP_OK) rc = R.rests();
    if (rc == MRP_OK) rc = R.filtered_front(sv_threshold);
    if (rc == MRP_OK) rc = R.anchors();
    if (rc == MRP_OK) rc = R.classify(forward_model, reverse_model, expansion);
    if (rc != MRP_OK) return rc;
    /* (made before anything is handed over: an error returns nothing) */
    R.fr_out.assign((size_t) n_chunks, nullptr);
    if (bubble_variant_out) R.bv_out.assign((size_t) n_chunks, nullptr);
    for (int64_t c = 0; c < n_chunks; c++) {
        std::vector<int32_t> fr = R.ra[(size_t) c].filtered_read;
        fr.push_back(-1); /* the end of the list */
        R.fr_out[(size_t) c] = (int32_t *) sc_dup(fr.data(), sizeof(int32_t) * fr.size());
        if (!R.fr_out[(size_t) c]) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
        if (!bubble_variant_out) continue;
        std::vector<int64_t> bv = R.arr[(size_t) c].bubble_variant;
        bv.push_back(-1);
        R.bv_out[(size_t) c] = (int64_t *) sc_dup(bv.data(), sizeof(int64_t) * bv.size());
        if (!R.bv_out[(size_t) c]) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int64_t c = 0; c < n_chunks; c++) out[c] = nullptr;
    if (profiles_out && n_chunks > 0) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    mrp_string_filtered_stats fst;
    memset(&fst, 0, sizeof(fst));
    if (n_chunks > 0) {
        R.F.front_ms = now_ms() - t_begin;
        rc = mrp_string_front_run(ctx, &R.F, het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out,
                                  stats ? &stats->aligned.chunks : nullptr, filtered_out, stats ? &fst : nullptr);
        if (rc != MRP_OK) return rc;
    }
    if (stats) {
        float ms = 0.f;
        if (R.cev[1]) PHM_HIP(hipEventElapsedTime(&ms, R.cev[0], R.cev[1]));
        stats->classes_ms = ms;
        stats->filtered_ms = fst.filtered_ms;
        stats->pairs_scored = fst.pairs_scored;
        stats->pairs_speculative = fst.pairs_speculative;
        stats->pairs_read_by_results = fst.pairs_read_by_results;
        stats->filtered_variants = R.D.n_variants - R.D.variant_first[n_chunks];
        stats->filtered_reads = R.n_filtered_reads;
        stats->filtered_entries = R.D.n_entries - (n_chunks > 0 ? R.k_first[R.D.variant_first[n_chunks]] : 0);
    }
    rc = R.hand_over(bubble_variant_out);
    if (rc != MRP_OK) return rc;
    R.d_ckey.release();
    R.d_rep.release();
    ctx->pool.reclaim();
    for (int64_t c = 0; c < n_chunks; c++) { filtered_read_out[c] = R.fr_out[(size_t) c]; R.fr_out[(size_t) c] = nullptr; }
    if (stats) stats->aligned.total_ms = now_ms() - t_begin;
    return MRP_OK;
}
