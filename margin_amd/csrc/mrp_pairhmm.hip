/*
 * mrp_pairhmm.hip -- read x allele alignment likelihoods: the banded pair-HMM forward probability of the reference
 * (computeForwardProbability, impl/pairwiseAligner.c:849-903) for batches of string pairs, and the alleleReadSupports
 * loop around it (impl/bubbleGraph.c:1421-1464), and the filtered-read / filtered-variant loops after the phasing
 * (:1749-2351: the supports stay on the device, a scoring kernel reduces them).  The string-chunk calls (mrp_string_chunks.hip) and the
 * composites over aligned chunks (mrp_aligned.hip) are built on it through mrp_pairhmm.h.  gfx950 only; compiled
 * with -ffp-contract=off.
 *
 * The recursion (stateMachine3_cellCalculate, impl/stateMachine.c:562-586) gives every dp cell (x, y) three states from
 * its neighbours (x-1, y), (x-1, y-1), (x, y-1); a neighbour outside the band contributes nothing, which is what a
 * neighbour holding LOG_ZERO contributes, so the kernels keep -inf where the reference keeps NULL.  Each state is a
 * chain of three logAdd (pairwiseAligner.c:279-299: cubic interpolation in fp64, float literals, no exp / log) in the
 * reference's order.  Three mappings:
 *
 *   phm_lane_kernel   a pair per LANE, for pairs whose x string has at most 100 symbols and no anchors (their band is
 *                     the whole matrix): the lane walks its matrix row by row, the previous row lives in LDS as
 *                     row[x][state][lane] (conflict-free), the column x = 0 in registers.  All 64 lanes do useful
 *                     work in every step when the pairs of a wave have similar shapes (the host sorts them), which
 *                     is the case that matters: margin phase aligns ~25-symbol alleles to ~25-symbol read substrings,
 *                     10^5 pairs per 1 Mb chunk.  LDS per wave = 1 536 B x (longest x string of the launch class):
 *                     25 symbols -> 4 waves per CU, one per SIMD.
 *   phm_wave_kernel   a pair per WAVE for everything else (long strings, anchored bands): x+y diagonal by diagonal, a
 *                     lane per cell of the diagonal, the last two diagonals in LDS -- up to 2 048 cells on a diagonal.
 *   phm_wide_kernel   a pair per WORKGROUP for the pairs beyond that, when the caller has turned wide pairs on (else they are
 *                     refused): the diagonals in a device workspace.  Both are the walk of mrp_pairhmm_walk.h, and
 *                     both exist a second time with the run-length emissions of margin polish (mrp_forward_probabilities_rle,
 *                     DESIGN.md 9.16).  So does phm_lane_kernel, for the unanchored pairs whose counts are all
 *                     below PHM_LANE_RLE_COUNTS: mrp_allele_read_supports_rle always sends them there, mrp_forward_probabilities_rle
 *                     once mrp_context_set_rle_lane_pairs is on; every other run-length pair keeps the two kernels above.
 *
 * Bound: fp64 VALU issue (six logAdd per cell); the kernels move ~0.1 B per flop.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_band.h"
#include "mrp_internal.h"
#include "mrp_pairhmm.h"
#include "mrp_pairhmm_walk.h" /* St, phm_log_add, phm_dot; the walk of the two diagonal kernels */
#include "mrp_wave.h"
#include "rphmm_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int PHM_LANE_MAX_X = 100;    /* 100 * 1 600 B = 156 KB of the 160 KB, the rest holds the tables */
constexpr int PHM_LDS_BYTES = 160 * 1024;
#define PHM_ROWS 2 /* rows a lane of the pair-per-lane kernel advances together (measured: 1 -> 2.49 ms, 2 -> 2.11, 3 -> 2.75, 4 -> 2.61, 6 -> 3.23 for 4.8e5 pairs) */
constexpr int PHM_LANE_BYTES_PER_X = 3 * 64 * 8 + 64; /* LDS per wave and x position: three states per lane + the lane's symbol */
constexpr int PHM_ETAB = 25 * 6;       /* doubles per model in the emission + transition table */
/* The run-length instantiation of the pair-per-lane kernel: a pair is eligible only if every count of both its strings
 * is below this bound, so that the part of the models' repeat tables a wave can ask for, rep_c[model][cx][u][o] with u, o below the
 * bound, lies in LDS beside the other tables (5 * 16 * 16 * 8 B = 10 240 B per model) and a symbol (0..4) with its count fits the byte
 * the row keeps per x position. */
constexpr int PHM_LANE_RLE_COUNTS = 16;
constexpr int PHM_LANE_RLE_REP = 5 * PHM_LANE_RLE_COUNTS * PHM_LANE_RLE_COUNTS; /* doubles per model in the compact repeat table */
static_assert(4 + ((PHM_LANE_RLE_COUNTS - 1) << 3) < 256, "a symbol and its count share a byte");

/* The tables of the pair-per-lane kernel in LDS, in doubles: coef | etab, and for run-length emissions em | rep_c behind them */
constexpr int phm_lane_table_doubles(int n_models, bool rle) { return 16 + n_models * (PHM_ETAB + (rle ? 25 + PHM_LANE_RLE_REP : 0)); }

/* The match emission of the pair-per-lane kernel, a policy as in the diagonal kernels (mrp_pairhmm_walk.h).  PhmLaneNucleotide: the
 * model's table, already summed with the three match transitions in etab.  PhmLaneRunLength: em[cx * 5 + cy] + rep_c[cx][u][o] added per
 * cell, then the transition (getRleNucleotideMatchProb, stateMachine.c:733-738; the association of phm_cell), both tables in LDS. */
struct PhmLaneNucleotide {
    static constexpr bool RLE = false;
    struct Args {};
};
struct PhmLaneRunLength {
    static constexpr bool RLE = true;
    struct Args {
        const uint8_t *counts; /* parallel to the symbol pool; every count of a lane pair is below PHM_LANE_RLE_COUNTS */
        const double *rep_c;   /* [model][cx][u][o], u, o < PHM_LANE_RLE_COUNTS: PhmRle::rep_lane */
    };
};

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

/* LDS: coef[16] | etab[n_models][cx][cy][6] = eX + {open, extend, switch to x}, eM + {continue, from x, from y} |
 * (run-length emissions only: em[n_models][cx][cy] | rep_c[n_models][cx][u][o]) | rows[wave][x - 1][state][lane].  The waves of a
 * workgroup share the tables and nothing else.  With run-length emissions the byte a row keeps per x position and the int a lane
 * keeps per y position hold symbol | count << 3; a slot that stands for no symbol holds 4 (N, count 0), so every table index of a
 * padding lane and of a cell beyond a lane's own strings is in range as well.
 *
 * A lane walks its matrix R rows at a time, row r one column behind row r - 1 (x_r = k - r in step k), so the R cells
 * of a step depend only on cells of earlier steps: left = the row's own cell of step k - 1, up / diagonal = the cells
 * of the row above from steps k - 1 / k - 2, all in registers.  Only the first row of a pass reads the LDS row (the last
 * row of the previous pass) and only the last row writes it.  With one wave per SIMD this is what hides the latency of
 * the dependent fp64 chains and of the table reads: R * 3 independent chains per step instead of 3.
 * Cells beyond a lane's own strings are computed and ignored: nothing flows from larger x or y to smaller. */
template <int R, bool HAS_SWITCH, class Em>
__global__ void __launch_bounds__(256) phm_lane_kernel(const PhmLanePair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                       const PhmModelDev *__restrict__ models, int n_models, int cap, double *__restrict__ out,
                                                       typename Em::Args ea) {
    extern __shared__ double phm_lds[];
    double *coef = phm_lds;
    double *etab = phm_lds + 16;
    const int lane = threadIdx.x & (PHM_WAVE - 1), wave = threadIdx.x / PHM_WAVE, n_waves = blockDim.x / PHM_WAVE;
    [[maybe_unused]] double *em_l = etab + (size_t) n_models * PHM_ETAB; /* run-length emissions: em | rep_c */
    [[maybe_unused]] double *rep_l = em_l + (size_t) n_models * 25;
    uint8_t *wave_base = reinterpret_cast<uint8_t *>(phm_lds + phm_lane_table_doubles(n_models, Em::RLE)) + (size_t) wave * cap * PHM_LANE_BYTES_PER_X;
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
        if constexpr (Em::RLE) em_l[i] = eM;
    }
    if constexpr (Em::RLE)
        for (int i = threadIdx.x; i < n_models * PHM_LANE_RLE_REP; i += blockDim.x) rep_l[i] = ea.rep_c[i];
    __syncthreads();
    const int64_t pi = ((int64_t) blockIdx.x * n_waves + wave) * PHM_WAVE + lane;
    const bool have = pi < n_pairs;
    PhmLanePair p;
    if (have) p = pairs[pi];
    else { p.x_off = 0; p.y_off = 0; p.lx = -1; p.ly = -1; p.model = 0; p.out = 0; }
    const int lx = p.lx, ly = p.ly;
    const int mx = wave_max_i32(lx), my = wave_max_i32(ly);
    const int mx1 = mx > 1 ? mx : 1;
    const PhmModelDev *__restrict__ M = models + p.model;
    const double t_open_y = M->t[4], t_extend_y = M->t[6], t_switch_y = M->t[8];
    const uint8_t *__restrict__ sx = pool + p.x_off;
    const uint8_t *__restrict__ sy = pool + p.y_off;
    /* symbol i of a string, with run-length emissions | its count << 3 */
    const auto sym_of = [&](const uint8_t *__restrict__ str, int64_t off, int i) {
        int c = str[i];
        c = c > 4 ? 4 : c;
        if constexpr (Em::RLE) c |= (int) ea.counts[off + i] << 3;
        return c;
    };
    [[maybe_unused]] double t_match[3] = {0.0, 0.0, 0.0};
    if constexpr (Em::RLE) { t_match[0] = M->t[0]; t_match[1] = M->t[1]; t_match[2] = M->t[2]; }
    /* no global loads inside the step loop (the compiler waits for each one on the spot): the x string goes to LDS */
    for (int x = 1; x <= mx1; x++) {
        int c = 4;
        if (x <= lx) c = sym_of(sx, p.x_off, x - 1);
        symx[(x - 1) * PHM_WAVE] = (uint8_t) c;
#pragma unroll
        for (int s = 0; s < 3; s++) row[((x - 1) * 3 + s) * PHM_WAVE] = PHM_NEG;
    }
    const St neg{PHM_NEG, PHM_NEG, PHM_NEG};
    St b_prev = neg; /* cell (0, y0 - 1) */
    St fin = neg;    /* cell (lx, ly) */
    const double *__restrict__ etab_m = etab + (size_t) p.model * PHM_ETAB;
    [[maybe_unused]] const double *__restrict__ em_m = em_l + (size_t) p.model * 25;
    [[maybe_unused]] const double *__restrict__ rep_m = rep_l + (size_t) p.model * PHM_LANE_RLE_REP;
    int cy_next[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        cy_next[r] = 4;
        if (r >= 1 && r <= ly) cy_next[r] = sym_of(sy, p.y_off, r - 1);
    }
    for (int y0 = 0; y0 <= my; y0 += R) {
        const double *etab_r[R];
        [[maybe_unused]] const double *em_r[R], *rep_r[R]; /* run-length emissions: the row's column of em and of rep_c */
        double ty_open[R], ty_extend[R], ty_switch[R];
        St b0[R]; /* cell (0, y0 + r): only the gap-y state can be reached */
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int y = y0 + r;
            const int cy = Em::RLE ? cy_next[r] & 7 : cy_next[r];
            if constexpr (Em::RLE) {
                em_r[r] = em_m + cy;
                rep_r[r] = rep_m + (cy_next[r] >> 3);
            }
            /* the y symbols of the next pass are requested now and waited for after the step loop */
            cy_next[r] = 4;
            if (y + R <= ly) cy_next[r] = sym_of(sy, p.y_off, y + R - 1);
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
                St cur;
                if constexpr (Em::RLE) {
                    const int cx = cxs[r] & 7, u = cxs[r] >> 3;
                    const double2 *__restrict__ e = reinterpret_cast<const double2 *>(etab_r[r] + cx * 30);
                    const double2 e01 = e[0];
                    const double e2 = etab_r[r][cx * 30 + 2];
                    const double eM = em_r[r][cx * 5] + rep_r[r][(cx * PHM_LANE_RLE_COUNTS + u) * PHM_LANE_RLE_COUNTS];
                    cur.x = phm_chain_t<HAS_SWITCH>(left.m + e01.x, left.x + e01.y, left.y + e2, coef);
                    cur.m = phm_chain_t<true>(diag.m + (eM + t_match[0]), diag.x + (eM + t_match[1]), diag.y + (eM + t_match[2]), coef);
                } else {
                    const double2 *__restrict__ e = reinterpret_cast<const double2 *>(etab_r[r] + cxs[r] * 30);
                    const double2 e01 = e[0], e23 = e[1], e45 = e[2];
                    cur.x = phm_chain_t<HAS_SWITCH>(left.m + e01.x, left.x + e01.y, left.y + e23.x, coef);
                    cur.m = phm_chain_t<true>(diag.m + e23.y, diag.x + e45.x, diag.y + e45.y, coef);
                }
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

/* A pair per WAVE (a workgroup of one wave): the walk of mrp_pairhmm_walk.h with the three live diagonals in LDS, 3 diagonals x W
 * cells x 3 states, then the total on the last diagonal.  Em: the match emission (PhmNucleotide, PhmRunLength), ea what it reads. */
template <class Em>
__global__ void __launch_bounds__(PHM_WAVE) phm_wave_kernel(const PhmPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                              const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band, int W,
                                                              double *__restrict__ out, typename Em::Args ea) {
    extern __shared__ double phm_diag[];
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PhmPair p = pairs[pi];
        const int n = p.lx + p.ly;
        if (n == 0) {
            if (threadIdx.x == 0) out[p.out] = 0.0; /* :860-862 */
            continue;
        }
        const PhmPairCtxT<Em> c = phm_pair_ctx<Em>(models, p.model, pool, p.x_off, p.y_off, ea);
        PhmDiagonals<PhmInterleaved, PHM_KEEP_NONE> diag{PhmInterleaved::at(phm_diag, W, 0), PhmInterleaved::at(phm_diag, W, 1), PhmInterleaved::at(phm_diag, W, 2)};
        const PhmBandOrMatrixLimits limits{band, p.band_off, p.lx, p.ly};
        phm_forward_walk<PhmTeam<PHM_WAVE, false>>(n, diag, limits, c);
        if (threadIdx.x == 0) out[p.out] = phm_last_diagonal_total(diag.d1, (diag.r1 - diag.l1) / 2, c.M);
        __syncthreads(); /* the next pair starts over in the diagonals that thread 0 has just read */
    }
}

/* A pair per WORKGROUP, for the pairs whose widest diagonal does not fit the LDS of phm_wave_kernel (wide pairs on): the same walk by
 * T threads.  The three live diagonals lie in the workgroup's slice of a device workspace, ws[workgroup][diagonal][state][W] (W = the
 * widest diagonal of the launch), and rotate by pointer.  A workgroup reads only what it wrote itself and runs on one CU: one
 * __syncthreads() between diagonals is the only synchronisation.  The next pair of the grid-stride loop reuses the slice; every
 * cell read lies inside [l1, r1] / [l2, r2] of the pair's own diagonals, which that pair wrote.  (No pair with an empty matrix
 * reaches this kernel; the walk would give it its start cell's total.) */
template <int T, class Em>
__global__ void __launch_bounds__(T) phm_wide_kernel(const PhmPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                     const PhmModelDev *__restrict__ models, const int32_t *__restrict__ band, int W, double *ws,
                                                     double *__restrict__ out, typename Em::Args ea) {
    double *slice = ws + (size_t) blockIdx.x * 9 * (size_t) W;
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const PhmPair p = pairs[pi];
        const PhmPairCtxT<Em> c = phm_pair_ctx<Em>(models, p.model, pool, p.x_off, p.y_off, ea);
        PhmDiagonals<PhmSlice, PHM_KEEP_NONE> diag{PhmSlice::at(slice, W, 0), PhmSlice::at(slice, W, 1), PhmSlice::at(slice, W, 2)};
        const int n = p.lx + p.ly;
        const PhmBandOrMatrixLimits limits{band, p.band_off, p.lx, p.ly};
        phm_forward_walk<PhmTeam<T, false>>(n, diag, limits, c);
        if (threadIdx.x == 0) out[p.out] = phm_last_diagonal_total(diag.d1, (diag.r1 - diag.l1) / 2, c.M);
        __syncthreads();
    }
}
constexpr int PHM_WIDE_THREADS = 1024; /* workgroup of phm_wide_kernel (measured against 256 and 512: DESIGN.md 9.10) */

}  // namespace

/* ---------------- host ---------------- */

/* band_construct in closed form (mrp_band.h, which also states band_constructDynamic) */
int band_closed_form(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, int64_t expansion, int32_t *L, int32_t *R,
                     int64_t *cells, int *max_width) {
    return band_closed_form_any(anchors, nullptr, false, n_anchors, lx, ly, expansion, L, R, cells, max_width);
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

/* wide pairs on: the two refusals that remain (what: "pair 12", "chunk 3: a pair of bubble 7") */
int phm_wide_caps(const char *who, const char *what, int64_t width, int64_t cells) {
    if (width > MRP_WIDE_MAX_WIDTH)
        return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: %s has a diagonal of %lld cells (limit %d with wide pairs on, MRP_WIDE_MAX_WIDTH)", who, what,
                             (long long) width, (int) MRP_WIDE_MAX_WIDTH);
    if (cells > MRP_WIDE_MAX_CELLS)
        return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: %s has %lld dp cells inside its band, its widest diagonal %lld (limit %lld cells with wide pairs on, MRP_WIDE_MAX_CELLS)",
                             who, what, (long long) cells, (long long) width, (long long) MRP_WIDE_MAX_CELLS);
    return MRP_OK;
}

/* The x-length caps of the four launch classes of the pair-per-lane kernel (4, 3, 2, 1 waves per workgroup) for n_models models, from
 * the LDS its tables leave; -1 throughout where they leave no room for a row (every pair then goes to the pair-per-wave kernel).  rle:
 * the tables of the run-length instantiation.  Returns the bytes of the tables. */
int phm_lane_caps(int n_models, bool rle, int cap[4]) {
    const int64_t table_bytes = (int64_t) phm_lane_table_doubles(n_models, rle) * (int64_t) sizeof(double);
    const int64_t left = PHM_LDS_BYTES - table_bytes;
    const int lane_max_x = left < PHM_LANE_BYTES_PER_X ? -1 : (int) std::min<int64_t>(PHM_LANE_MAX_X, left / PHM_LANE_BYTES_PER_X);
    for (int c = 0; c < 4; c++) cap[c] = lane_max_x < 0 ? -1 : (int) std::min<int64_t>(lane_max_x, left / ((4 - c) * PHM_LANE_BYTES_PER_X));
    return (int) std::min<int64_t>(table_bytes, INT32_MAX);
}

/* The host half of a pair-HMM batch of n_pairs > 0 pairs, no device needed: the pairs sorted into the launch classes of
 * the two kernels, the bands of the anchored ones, the models as the kernels read them.  Every error of the batch (prefixed
 * with who) is raised here, MRP_ERR_UNSUPPORTED for a diagonal beyond PHM_WAVE_MAX_WIDTH cells among them -- or, with wide_pairs,
 * beyond the caps of the pair-per-workgroup kernel, which then takes the pairs beyond PHM_WAVE_MAX_WIDTH (L.wide_pairs). */
int phm_classify(const char *who, const mrp_pair_hmm *models, int32_t n_models, int64_t pool_bytes, const PhmPairs &P, int64_t expansion,
                 int ragged_left, int ragged_right, int wide_pairs, PhmLaunch &L) {
    const int64_t n_pairs = P.n;
    const int64_t *x_off = P.x_off, *y_off = P.y_off, *anchor_off = P.anchor_off, *anchors = P.anchors;
    const int32_t *x_len = P.x_len, *y_len = P.y_len;
    const uint8_t *model_index = P.model;
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);

    /* classify.  The pair-per-lane kernel takes the unanchored pairs whose x string fits its LDS row next to the tables;
     * launch classes by x length (4, 3, 2, 1 waves per workgroup = per CU).  A run-length batch (L.rle) has lane classes only
     * if L.rle_lane is on, and then for the pairs whose counts are all below PHM_LANE_RLE_COUNTS. */
    const bool rle = L.rle != nullptr;
    int lane_cap[4];
    const int table_bytes = phm_lane_caps(n_models, rle, lane_cap);
    if (rle && !L.rle_lane)
        for (int c = 0; c < 4; c++) lane_cap[c] = -1;
    const int lane_max_x = lane_cap[3];
    const uint8_t *rle_counts = rle ? L.rle->counts : nullptr;
    const auto counts_below_bound = [rle_counts](int64_t off, int64_t len) {
        for (int64_t k = 0; k < len; k++)
            if (rle_counts[off + k] >= PHM_LANE_RLE_COUNTS) return false;
        return true;
    };
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
            if (na == 0 && lx <= lane_max_x && (!rle || (counts_below_bound(x_off[i], lx) && counts_below_bound(y_off[i], ly)))) {
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
        int64_t pair_cells;
        if (na == 0) {
            width = (int) std::min(lx, ly) + 1;
            pair_cells = (lx + 1) * (ly + 1);
            cells += pair_cells;
        } else {
            if (lx + ly >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who);
            Lb.resize((size_t) (lx + ly + 1));
            Rb.resize((size_t) (lx + ly + 1));
            int64_t c = 0;
            const int rc = band_closed_form(anchors + 2 * anchor_off[i], na, lx, ly, expansion, Lb.data(), Rb.data(), &c, &width);
            if (rc != MRP_OK) return mrp_set_error(rc, "%s: pair %lld has invalid anchors (pairwiseAligner.c:206-211)", who, (long long) i);
            cells += c;
            pair_cells = c;
            p.band_off = (int64_t) band.size() / 2;
            for (int64_t d = 0; d <= lx + ly; d++) { band.push_back(Lb[(size_t) d]); band.push_back(Rb[(size_t) d]); }
        }
        if (width > PHM_WAVE_MAX_WIDTH) {
            if (!wide_pairs)
                return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: pair %lld has a diagonal of %d cells (limit %d)", who, (long long) i, width, PHM_WAVE_MAX_WIDTH);
            char what[48];
            snprintf(what, sizeof(what), "pair %lld", (long long) i);
            const int rc = phm_wide_caps(who, what, width, pair_cells);
            if (rc != MRP_OK) return rc;
            L.wide_pairs.push_back(p);
            L.wide_width = std::max(L.wide_width, width);
            L.wide_cells += pair_cells;
            continue;
        }
        int c = 0;
        while (width > WAVE_CLASS_CAP[c]) c++;
        wave_pairs[c].push_back(p);
    }
    const auto largest_first = [](const PhmPair &a, const PhmPair &b) {
        const int64_t ca = (int64_t) a.lx * a.ly, cb = (int64_t) b.lx * b.ly;
        return ca != cb ? ca > cb : a.out < b.out;
    };
    for (int c = 0; c < 4; c++) std::sort(wave_pairs[c].begin(), wave_pairs[c].end(), largest_first);
    std::sort(L.wide_pairs.begin(), L.wide_pairs.end(), largest_first);
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
                const uint8_t *device_pool) {
    const int n_models = H.n_models, table_bytes = H.table_bytes;
    const bool has_switch = H.has_switch;
    const HostVec<PhmLanePair> *lane_pairs = H.lane_pairs;
    const HostVec<PhmPair> *wave_pairs = H.wave_pairs;
    const HostVec<int32_t> &band = H.band;
    PHM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    L.arrays.bind(&ctx->pool);
    L.s = s; /* from here on the destructor drains the stream */
    PHM_HIP(L.d_models.upload(H.hm, s));
    if (!device_pool) {
        PHM_HIP(L.d_pool.alloc((size_t) pool_bytes));
        if (pool_bytes) PHM_HIP(hipMemcpyAsync(L.d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, s));
        device_pool = L.d_pool.p;
    }
    PHM_HIP(L.d_band.upload(band, s));
    PHM_HIP(L.d_out.alloc((size_t) n_pairs));
    if (H.rle) PHM_HIP(L.rle.upload(&ctx->pool, *H.rle, pool_bytes, s));
    bool rle_lane_pairs = false;
    for (int c = 0; c < 4; c++) rle_lane_pairs = rle_lane_pairs || (H.rle && !lane_pairs[c].empty());
    if (rle_lane_pairs) PHM_HIP(L.rle.d_rep_lane.upload(H.rle->rep_lane, s)); /* (no lane pair: nothing beyond what the pair-per-wave kernel reads goes up) */
    for (int c = 0; c < 4; c++) {
        PHM_HIP(L.d_lane[c].upload(lane_pairs[c], s));
        PHM_HIP(L.d_wave[c].upload(wave_pairs[c], s));
    }
    /* the pair-per-workgroup kernel: as many workgroups as the workspace bound holds slices of 9 x (widest diagonal) doubles */
    const int64_t n_wide = (int64_t) H.wide_pairs.size();
    int64_t wide_grid = 0;
    if (n_wide > 0) {
        const int64_t slice_bytes = 9 * (int64_t) H.wide_width * (int64_t) sizeof(double);
        wide_grid = std::min(n_wide, std::max<int64_t>(1, PHM_WIDE_WORKSPACE_BYTES / slice_bytes));
        if (ctx->test_hooks & 64) wide_grid = 1; /* test hook: consecutive pairs reuse one slice */
        PHM_HIP(L.d_wide.upload(H.wide_pairs, s));
        PHM_HIP(L.d_wide_ws.alloc((size_t) wide_grid * 9 * (size_t) H.wide_width));
    }
    /* once per device (contexts of several host threads may call concurrently) */
    static PerDeviceOnce once;
    const hipError_t configured = once.run([] {
        hipError_t e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, true, PhmLaneNucleotide>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, false, PhmLaneNucleotide>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, true, PhmLaneRunLength>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *) phm_lane_kernel<PHM_ROWS, false, PhmLaneRunLength>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *) phm_wave_kernel<PhmNucleotide>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *) phm_wave_kernel<PhmRunLength>, hipFuncAttributeMaxDynamicSharedMemorySize, PHM_LDS_BYTES);
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
        const dim3 grid((unsigned) ((n + per_wg - 1) / per_wg)), block((unsigned) per_wg);
        if (H.rle) {
            const PhmLaneRunLength::Args ea{L.rle.d_counts.p, L.rle.d_rep_lane.p};
            if (has_switch)
                hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, true, PhmLaneRunLength>), grid, block, lds, s, L.d_lane[c].p, n, device_pool, L.d_models.p, (int) n_models,
                                   cap, L.d_out.p, ea);
            else
                hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, false, PhmLaneRunLength>), grid, block, lds, s, L.d_lane[c].p, n, device_pool, L.d_models.p, (int) n_models,
                                   cap, L.d_out.p, ea);
        } else if (has_switch)
            hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, true, PhmLaneNucleotide>), grid, block, lds, s, L.d_lane[c].p, n, device_pool, L.d_models.p, (int) n_models, cap,
                               L.d_out.p, PhmLaneNucleotide::Args{});
        else
            hipLaunchKernelGGL((phm_lane_kernel<PHM_ROWS, false, PhmLaneNucleotide>), grid, block, lds, s, L.d_lane[c].p, n, device_pool, L.d_models.p, (int) n_models, cap,
                               L.d_out.p, PhmLaneNucleotide::Args{});
        PHM_HIP(hipGetLastError());
        if (stats) stats->pairs_lane += n;
    }
    for (int c = 0; c < 4; c++) {
        const int64_t n = (int64_t) wave_pairs[c].size();
        if (n == 0) continue;
        const int W = WAVE_CLASS_CAP[c];
        const size_t lds = (size_t) 9 * W * sizeof(double);
        const dim3 grid((unsigned) std::min<int64_t>(n, 16384));
        if (H.rle)
            hipLaunchKernelGGL(phm_wave_kernel<PhmRunLength>, grid, dim3(PHM_WAVE), lds, s, L.d_wave[c].p, n, device_pool, L.d_models.p, L.d_band.p, W, L.d_out.p,
                               PhmRunLength::Args{L.rle.d_counts.p, L.rle.d_models.p});
        else
            hipLaunchKernelGGL(phm_wave_kernel<PhmNucleotide>, grid, dim3(PHM_WAVE), lds, s, L.d_wave[c].p, n, device_pool, L.d_models.p, L.d_band.p, W, L.d_out.p,
                               PhmNucleotide::Args{});
        PHM_HIP(hipGetLastError());
        if (stats) stats->pairs_wave += n;
    }
    if (n_wide > 0) {
        if (H.rle)
            hipLaunchKernelGGL((phm_wide_kernel<PHM_WIDE_THREADS, PhmRunLength>), dim3((unsigned) wide_grid), dim3(PHM_WIDE_THREADS), 0, s, L.d_wide.p, n_wide, device_pool,
                               L.d_models.p, L.d_band.p, H.wide_width, L.d_wide_ws.p, L.d_out.p, PhmRunLength::Args{L.rle.d_counts.p, L.rle.d_models.p});
        else
            hipLaunchKernelGGL((phm_wide_kernel<PHM_WIDE_THREADS, PhmNucleotide>), dim3((unsigned) wide_grid), dim3(PHM_WIDE_THREADS), 0, s, L.d_wide.p, n_wide, device_pool,
                               L.d_models.p, L.d_band.p, H.wide_width, L.d_wide_ws.p, L.d_out.p, PhmNucleotide::Args{});
        PHM_HIP(hipGetLastError());
        if (stats) stats->pairs_wave += n_wide;
        ctx->wide_pair_count += n_wide;
        ctx->wide_cell_count += H.wide_cells;
    }
    return MRP_OK;
}

/* The MRP_ERR_ARG of the run-length entries, raised with the other argument errors, and the tables: rep = 2.3025 * log_prob, one IEEE
 * multiply per entry (getRleNucleotideMatchProb, stateMachine.c:733-738), rows by x symbol with the strand and N rules of
 * repeatSubMatrix_setLogProb (repeatSubMatrix.c:16-29).  P's offsets and model indices have been checked by the caller. */
static int phm_rle_check_models(const char *who, const mrp_repeat_model *repeat, int32_t n_models) {
    if (!repeat) return mrp_set_error(MRP_ERR_ARG, "%s: repeat is NULL", who);
    for (int32_t m = 0; m < n_models; m++) {
        if (!repeat[m].log_prob) return mrp_set_error(MRP_ERR_ARG, "%s: repeat model %d has no log_prob", who, (int) m);
        if (repeat[m].max_repeat < 2 || repeat[m].max_repeat > 256)
            return mrp_set_error(MRP_ERR_ARG, "%s: repeat model %d: max_repeat %d outside [2, 256]", who, (int) m, (int) repeat[m].max_repeat);
        if (repeat[m].strand != 0 && repeat[m].strand != 1) return mrp_set_error(MRP_ERR_ARG, "%s: repeat model %d: strand must be 0 or 1", who, (int) m);
    }
    return MRP_OK;
}
int phm_rle_check_and_build(const char *who, const mrp_repeat_model *repeat, int32_t n_models, const uint8_t *counts, const PhmPairs &P, PhmRle &out) {
    const int rc = phm_rle_check_models(who, repeat, n_models);
    if (rc != MRP_OK) return rc;
    bool any = false;
    for (int64_t i = 0; i < P.n && !any; i++) any = P.x_len[i] > 0 || P.y_len[i] > 0;
    if (any && !counts) return mrp_set_error(MRP_ERR_ARG, "%s: counts is NULL", who);
    for (int64_t i = 0; i < P.n; i++) {
        const int R = repeat[P.model ? P.model[i] : 0].max_repeat;
        const int64_t off[2] = {P.x_off[i], P.y_off[i]}, len[2] = {P.x_len[i], P.y_len[i]};
        for (int q = 0; q < 2; q++)
            for (int64_t k = 0; k < len[q]; k++)
                if (counts[off[q] + k] >= R)
                    return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld: the count %d of %c symbol %lld is not below max_repeat %d of its model", who, (long long) i,
                                         (int) counts[off[q] + k], q ? 'y' : 'x', (long long) k, R);
    }
    out.counts = counts;
    out.rep.clear();
    out.rep_first.clear();
    out.R.clear();
    for (int32_t m = 0; m < n_models; m++) {
        const int64_t R = repeat[m].max_repeat;
        out.rep_first.push_back((int64_t) out.rep.size());
        out.R.push_back((int32_t) R);
        for (int cx = 0; cx < 5; cx++) {
            const int base = cx >= 4 ? 0 : cx;
            const double *src = repeat[m].log_prob + (repeat[m].strand ? base : 3 - base) * R * R;
            for (int64_t k = 0; k < R * R; k++) out.rep.push_back(2.3025 * src[k]);
        }
    }
    /* what the pair-per-lane kernel keeps in LDS: the same products for the counts below its bound (0 where the model has none) */
    out.rep_lane.assign((size_t) n_models * PHM_LANE_RLE_REP, 0.0);
    for (int32_t m = 0; m < n_models; m++) {
        const int64_t R = repeat[m].max_repeat, B = std::min<int64_t>(R, PHM_LANE_RLE_COUNTS);
        const double *full = out.rep.data() + out.rep_first[(size_t) m];
        double *compact = out.rep_lane.data() + (size_t) m * PHM_LANE_RLE_REP;
        for (int cx = 0; cx < 5; cx++)
            for (int64_t u = 0; u < B; u++)
                for (int64_t o = 0; o < B; o++) compact[(cx * PHM_LANE_RLE_COUNTS + u) * PHM_LANE_RLE_COUNTS + o] = full[(cx * R + u) * R + o];
    }
    return MRP_OK;
}

/* cachedScores of the reference's bubble loops (bubbleGraph.c:1418,1844,2221, keyed by the substring alone): for every
 * entry k of every group g (entries [first[g], first[g + 1])), owner[k] = the entry of the group whose scores k takes,
 * itself if it is scored.  Only entries with may_own[k] != 0 (NULL: all) take part; the others get owner -1 (not scored,
 * not cached).  last: among the entries of a group with equal substrings the last one owns the scores, else the first.
 * counts (NULL: none): an array parallel to pool; substrings are equal only if their counts are equal too (the run-length loops,
 * bubbleGraph.c:1042-1055). */
void substring_owners(int64_t n_groups, const int64_t *first, const uint8_t *pool, const int64_t *off, const int32_t *len,
                      const uint8_t *may_own, bool last, std::vector<int64_t> &owner, const uint8_t *counts) {
    owner.assign((size_t) first[n_groups], -1);
    mrp_parallel_for(n_groups, 64, [&](int64_t g) {
        std::vector<int64_t> order;
        for (int64_t k = first[g]; k < first[g + 1]; k++)
            if (!may_own || may_own[k]) order.push_back(k);
        /* (a substring of no symbols reads nothing: its offset may stand where the arrays end, or the arrays be NULL) */
        auto compare = [&](int64_t a, int64_t c) {
            if (len[a] == 0) return 0;
            const int cmp = memcmp(pool + off[a], pool + off[c], (size_t) len[a]);
            return cmp != 0 || !counts ? cmp : memcmp(counts + off[a], counts + off[c], (size_t) len[a]);
        };
        auto same = [&](int64_t a, int64_t c) { return len[a] == len[c] && compare(a, c) == 0; };
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t c) {
            if (len[a] != len[c]) return len[a] < len[c];
            const int cmp = compare(a, c);
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

namespace {

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

}  // namespace

int ht_partition_enqueue(mrp_context *ctx, hipStream_t s, const HostVec<int64_t> &first, const HostVec<HtEntry> &ent, const double *lp, int64_t n_reads,
                         HtPartitionDev &B) {
    B.arrays.bind(&ctx->pool);
    PHM_HIP(B.d_first.upload(first, s));
    PHM_HIP(B.d_ent.upload(ent, s));
    PHM_HIP(B.d_hap.alloc((size_t) n_reads));
    PHM_HIP(B.d_h.alloc(2 * (size_t) n_reads));
    if (n_reads > 0) {
        hipLaunchKernelGGL(ht_partition_kernel, dim3((unsigned) ((n_reads + 255) / 256)), dim3(256), 0, s, B.d_first.p, B.d_ent.p, lp, n_reads, B.d_hap.p, B.d_h.p,
                           B.d_h.p + n_reads);
        PHM_HIP(hipGetLastError());
    }
    PHM_HIP(hipEventRecord(ctx->ev[1], s));
    return MRP_OK;
}

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

int mrp_pair_diagonal_width(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, int64_t expansion, int32_t *width_out,
                            int64_t *cells_out) {
    if ((n_anchors > 0 && !anchors) || n_anchors < 0) return fail(MRP_ERR_ARG, "mrp_pair_diagonal_width: null argument");
    if (lx < 0 || ly < 0 || expansion < 0 || expansion % 2 != 0)
        return fail(MRP_ERR_ARG, "mrp_pair_diagonal_width: invalid anchors or expansion (pairwiseAligner.c:179,206-211)");
    if (lx + ly >= (1ll << 30)) return fail(MRP_ERR_ARG, "mrp_pair_diagonal_width: strings too long");
    int width = (int) std::min(lx, ly) + 1; /* no anchors: the whole matrix, as phm_classify counts it */
    int64_t cells = (lx + 1) * (ly + 1);
    if (n_anchors > 0) {
        std::vector<int32_t> Lb((size_t) (lx + ly + 1)), Rb((size_t) (lx + ly + 1));
        const int rc = band_closed_form(anchors, n_anchors, lx, ly, expansion, Lb.data(), Rb.data(), &cells, &width);
        if (rc != MRP_OK) return fail(rc, "mrp_pair_diagonal_width: invalid anchors or expansion (pairwiseAligner.c:179,206-211)");
    }
    if (width_out) *width_out = width;
    if (cells_out) *cells_out = cells;
    return MRP_OK;
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

int64_t mrp_rle_compress(const char *s, int64_t n, int32_t max_repeat, uint8_t *symbols_out, uint8_t *counts_out) {
    if (n < 0 || (n > 0 && (!s || !symbols_out || !counts_out)) || max_repeat < 2 || max_repeat > 256) return -1;
    int64_t m = 0;
    for (int64_t i = 0; i < n;) { /* rleString_construct, rle.c:7-38: a run of one character, compared as chars ("aA" is two runs) */
        int64_t j = i + 1;
        while (j < n && s[j] == s[i]) j++;
        mrp_symbols_from_chars(s + i, 1, symbols_out + m);
        const int64_t run = j - i;
        counts_out[m++] = (uint8_t) (run >= max_repeat ? max_repeat - 1 : run); /* symbol_addRepeatCount, stateMachine.c:124-131 */
        i = j;
    }
    return m;
}

int mrp_forward_probabilities_rle(mrp_context *ctx, const mrp_pair_hmm *models, const mrp_repeat_model *repeat, int32_t n_models, int64_t n_pairs,
                                  const uint8_t *pool, const uint8_t *counts, int64_t pool_bytes, const int64_t *x_off, const int32_t *x_len,
                                  const int64_t *y_off, const int32_t *y_len, const uint8_t *model_index, const int64_t *anchor_off, const int64_t *anchors,
                                  int64_t expansion, int ragged_left, int ragged_right, double *out, mrp_pairhmm_stats *stats) {
    static const char *who = "mrp_forward_probabilities_rle";
    const double t_begin = now_ms();
    /* the argument errors first, before the context is looked at; nothing is written on an error */
    if (n_pairs < 0 || n_models <= 0 || !models || pool_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (n_pairs > 0 && (!x_off || !x_len || !y_off || !y_len || !out || (pool_bytes > 0 && !pool))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    const PhmPairs P{n_pairs, x_off, x_len, y_off, y_len, model_index, anchor_off, anchors};
    for (int64_t i = 0; i < n_pairs; i++)
        if (x_len[i] < 0 || y_len[i] < 0 || x_off[i] < 0 || y_off[i] < 0 || x_off[i] + x_len[i] > pool_bytes || y_off[i] + y_len[i] > pool_bytes ||
            (model_index && model_index[i] >= n_models))
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld lies outside the symbol pool or names a model >= %d", who, (long long) i, (int) n_models);
    PhmRle rle;
    const int rc = phm_rle_check_and_build(who, repeat, n_models, counts, P, rle);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the pair-HMM path has no CPU fallback)", who);
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_pairs == 0) return MRP_OK;
    return phm_call(
        ctx, who, models, n_models, pool, pool_bytes, P, expansion, ragged_left, ragged_right, stats, t_begin,
        [&](hipStream_t s, const double *lp) {
            PHM_HIP(hipEventRecord(ctx->ev[1], s));
            PHM_HIP(hipMemcpyAsync(out, lp, (size_t) n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
            return (int) MRP_OK;
        },
        &rle, ctx->rle_lane_pairs != 0);
}

int mrp_rle_lane_caps(int32_t n_models, int32_t cap_out[4], int32_t *count_bound_out) {
    if (n_models <= 0) return fail(MRP_ERR_ARG, "mrp_rle_lane_caps: n_models must be positive");
    int cap[4];
    (void) phm_lane_caps(n_models, true, cap);
    if (cap_out)
        for (int c = 0; c < 4; c++) cap_out[c] = cap[c];
    if (count_bound_out) *count_bound_out = PHM_LANE_RLE_COUNTS;
    return MRP_OK;
}

int mrp_allele_read_supports_rle(mrp_context *ctx, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                 const mrp_repeat_model *forward_repeat, const mrp_repeat_model *reverse_repeat, int64_t n_bubbles,
                                 const int64_t *allele_first, const int64_t *read_first, const uint8_t *pool, const uint8_t *counts, int64_t pool_bytes,
                                 const int64_t *allele_off, const int32_t *allele_len, const int64_t *read_off, const int32_t *read_len,
                                 const uint8_t *read_forward_strand, int64_t expansion, float *support, mrp_pairhmm_stats *stats) {
    static const char *who = "mrp_allele_read_supports_rle";
    const double t_begin = now_ms();
    /* the argument errors first, before the context is looked at; nothing is written on an error */
    if (n_bubbles < 0 || pool_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (!forward_model || !reverse_model || !forward_repeat || !reverse_repeat || (pool_bytes > 0 && !pool))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (n_bubbles > 0 && (!allele_first || !read_first)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (n_bubbles > 0 && (allele_first[0] != 0 || read_first[0] != 0)) return mrp_set_error(MRP_ERR_ARG, "%s: offsets must start at 0", who);
    std::vector<int64_t> support_first((size_t) n_bubbles + 1, 0);
    for (int64_t b = 0; b < n_bubbles; b++) {
        const int64_t na = allele_first[b + 1] - allele_first[b], nr = read_first[b + 1] - read_first[b];
        if (na < 0 || nr < 0) return mrp_set_error(MRP_ERR_ARG, "%s: offsets not ascending at bubble %lld", who, (long long) b);
        support_first[(size_t) b + 1] = support_first[(size_t) b] + na * nr;
    }
    const int64_t n_alleles = n_bubbles ? allele_first[n_bubbles] : 0, n_reads = n_bubbles ? read_first[n_bubbles] : 0;
    if ((n_alleles > 0 && (!allele_off || !allele_len)) || (n_reads > 0 && (!read_off || !read_len || !read_forward_strand)) ||
        (support_first[(size_t) n_bubbles] > 0 && !support))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    bool any_symbol = false;
    for (int64_t j = 0; j < n_alleles; j++) {
        if (allele_len[j] < 0 || allele_off[j] < 0 || allele_off[j] + allele_len[j] > pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: allele %lld lies outside the pool", who, (long long) j);
        any_symbol = any_symbol || allele_len[j] > 0;
    }
    for (int64_t k = 0; k < n_reads; k++) {
        if (read_len[k] < 0 || read_off[k] < 0 || read_off[k] + read_len[k] > pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: read substring %lld lies outside the pool", who, (long long) k);
        any_symbol = any_symbol || read_len[k] > 0;
    }
    if (any_symbol && !counts) return mrp_set_error(MRP_ERR_ARG, "%s: counts is NULL", who);
    if (expansion < 0 || expansion % 2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: diagonalExpansion must be even (pairwiseAligner.c:855)", who);
    const mrp_pair_hmm models[2] = {*forward_model, *reverse_model};
    const mrp_repeat_model repeat[2] = {*forward_repeat, *reverse_repeat}; /* model 0: forward strand reads, model 1: reverse */
    int rc = phm_rle_check_models(who, repeat, 2);
    if (rc != MRP_OK) return rc;
    /* cachedScores (:1042-1065): the first read of the bubble with a given substring, symbols and counts, owns the scores */
    std::vector<int64_t> owner;
    if (n_bubbles > 0) substring_owners(n_bubbles, read_first, pool, read_off, read_len, nullptr, false, owner, counts);
    /* a count is checked against the model its string is scored with: a read's own strand's, an allele's for every strand among its
     * bubble's owners */
    const auto bad_count = [&](int64_t off, int64_t len, int R) {
        for (int64_t i = 0; i < len; i++)
            if (counts[off + i] >= R) return i;
        return (int64_t) -1;
    };
    PhmPairList pairs;
    std::vector<int64_t> where;
    for (int64_t b = 0; b < n_bubbles; b++) {
        const int64_t nr = read_first[b + 1] - read_first[b];
        bool strand_owns[2] = {false, false};
        for (int64_t k = read_first[b]; k < read_first[b + 1]; k++) {
            if (owner[(size_t) k] != k) continue;
            const int mi = read_forward_strand[k] ? 0 : 1;
            strand_owns[mi] = true;
            const int64_t i = bad_count(read_off[k], read_len[k], repeat[mi].max_repeat);
            if (i >= 0)
                return mrp_set_error(MRP_ERR_ARG, "%s: bubble %lld: the count %d of symbol %lld of read %lld is not below max_repeat %d of its strand's model", who,
                                     (long long) b, (int) counts[read_off[k] + i], (long long) i, (long long) (k - read_first[b]), (int) repeat[mi].max_repeat);
            for (int64_t j = allele_first[b]; j < allele_first[b + 1]; j++) {
                where.push_back(support_first[(size_t) b] + (j - allele_first[b]) * nr + (k - read_first[b]));
                pairs.add(allele_off[j], allele_len[j], read_off[k], read_len[k], mi, nullptr);
            }
        }
        for (int mi = 0; mi < 2; mi++) {
            if (!strand_owns[mi]) continue;
            for (int64_t j = allele_first[b]; j < allele_first[b + 1]; j++) {
                const int64_t i = bad_count(allele_off[j], allele_len[j], repeat[mi].max_repeat);
                if (i >= 0)
                    return mrp_set_error(MRP_ERR_ARG, "%s: bubble %lld: the count %d of symbol %lld of allele %lld is not below max_repeat %d of the %s strand's model",
                                         who, (long long) b, (int) counts[allele_off[j] + i], (long long) i, (long long) (j - allele_first[b]),
                                         (int) repeat[mi].max_repeat, mi ? "reverse" : "forward");
            }
        }
    }
    if (pairs.size() >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs in one call", who);
    const PhmPairs P = pairs.view();
    PhmRle rle;
    rc = phm_rle_check_and_build(who, repeat, 2, counts, P, rle);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the pair-HMM path has no CPU fallback)", who);
    if (stats) memset(stats, 0, sizeof(*stats));
    if (P.n == 0) return MRP_OK;
    std::vector<double> lp((size_t) P.n);
    rc = phm_call(
        ctx, who, models, 2, pool, pool_bytes, P, expansion, 0, 0, stats, t_begin,
        [&](hipStream_t s, const double *d_lp) {
            PHM_HIP(hipEventRecord(ctx->ev[1], s));
            PHM_HIP(hipMemcpyAsync(lp.data(), d_lp, (size_t) P.n * sizeof(double), hipMemcpyDeviceToHost, s));
            return (int) MRP_OK;
        },
        &rle, true); /* eligible pairs always run a pair per lane */
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
        HtPartitionDev B;
        const int rc = ht_partition_enqueue(ctx, s, first, ent, lp, n_reads, B);
        if (rc != MRP_OK) return rc;
        PHM_HIP(hipMemcpyAsync(hap, B.d_hap.p, (size_t) n_reads * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h1, B.d_h.p, (size_t) n_reads * sizeof(double), hipMemcpyDeviceToHost, s));
        PHM_HIP(hipMemcpyAsync(h2, B.d_h.p + n_reads, (size_t) n_reads * sizeof(double), hipMemcpyDeviceToHost, s));
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

}  // extern "C"
