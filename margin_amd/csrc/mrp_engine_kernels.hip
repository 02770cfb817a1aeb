/*
 * mrp_engine_kernels.hip -- the prune of a device-resident merge level.  The level's other stages: mrp_engine_cross.hip
 * (cross product, + emission), mrp_engine_layout.hip (column structure, layout), mrp_engine_small.hip (one-wave hmms, compaction),
 * mrp_engine_final.hip (trace back, genome fragments).  Shared: mrp_wave.h, mrp_cross_cells.h, mrp_prune_rule.h.
 *
 *  mrp_prune_kernel    stRPHmm_prune (hmm.c:1049-1163): pruneForwards walks the columns keeping the
 *                      best linked cells and merge cells by posterior (stable order on ties),
 *                      pruneBackwards (mrp_prune_back_kernel) removes what became unreachable.  Max-plus mode
 *                      only: the posterior exp(f + b - total) is monotone in the integer f + b - total, which
 *                      is what is ranked (bins; everything at or below the underflow point of exp
 *                      shares the last bin, exactly as equal doubles tie in the reference).
 */
#include <type_traits>

#include "mrp_engine.h"
#include "mrp_internal.h" /* PerDeviceOnce */
#include "mrp_level_order.h" /* prune_class, prune_lds_bytes, PRUNE_SP, PRUNE_TAB */
#include "mrp_cross_cells.h"
#include "mrp_prune_rule.h"
#include "mrp_wave.h"

/*
 * stRPHmm_prune for the cross products of a level, one workgroup per hmm.
 *
 * What the forward pass (stRPHmm_pruneForwards, hmm.c:1049-1109) needs of a column is small: the cells LINKED to a kept
 * merge cell of the previous merge column -- typically a hundred or two of the column's thousands (the cells of a cross
 * product column are all pairs (c1, c2) of the parents' cells; a kept merge cell (i, j) links exactly the pairs with
 * prev(c1) = i and prev(c2) = j).  So the candidates are ENUMERATED from the <= 128 kept merge cells and the parents'
 * transition arrays (<= 128 entries per side, inverted into per-merge-cell lists), never searched for among the cells:
 *
 *   wave 0        the sequential chain, without a barrier inside a column: kept merge cells -> candidates (64 per slot, as
 *                 many slots as the column needs; cell index by the closed form of the cross product order) -> posterior
 *                 bins (LDS gathers) -> cutoff bin by histogram -> selection (ties in the cutoff bin by list order = cell
 *                 index, ranked through a bitmap) -> the distinct next merge cells of the selection = the kept merge cells
 *                 of the next column, listed with their per-side indices.
 *   wave 1, 2     one and two columns behind: stable sort of the selection, kept lists to HBM, posteriors of the merge
 *                 cells, kept merge list (stRPHmm_pruneForwards' list building; nothing on the chain reads it).
 *   wave 3        inverts the parents' prev arrays of the NEXT column (loaded one column earlier), zeroes the histogram.
 *   waves 4..     two groups alternating over the columns: stream f and b of a whole column (the only bulk traffic: 8 B
 *                 per cell, requested two columns ahead) and leave its posterior bins in LDS as 16-bit values.
 *
 * Selection, tie order and list contents are those of the reference: sorting by (bin, cell index) is the stable sort of
 * the linked cells (in list order) by descending posterior (hmm.c:1043, :1071).
 */
struct PruneIn {
    const SweepCol *scols;
    const CrossCol *ccols;
    const int32_t *cell_f32, *cell_b32, *merge_f32, *merge_b32;
    const double *hmm_fb;
};

/* buffer descriptor over [p, p + bytes): both made wave-uniform for the compiler (cdna_hip_programming.md T8 / T20) */
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t prune_rsrc(const void *p, int bytes) {
    const uint64_t a = (uint64_t) p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) a), hi = __builtin_amdgcn_readfirstlane((uint32_t) (a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *) (((uint64_t) hi << 32) | lo), 0, bytes, 0x00020000);
}

/* profiling aid: build with -DPRUNE_EXP_CLOCK (both mrp_engine.cpp and this file) to sum, for the first hmm of a launch, the
 * shader cycles each role spends working and waiting at the column barrier (printed by mrp_engine.cpp under MRP_TIMING) */
#ifdef PRUNE_EXP_CLOCK
#define ROLE_CLK_INIT() uint64_t clk_work = 0, clk_wait = 0, clk_t = __builtin_amdgcn_s_memtime()
#define ROLE_BARRIER() do { const uint64_t t1_ = __builtin_amdgcn_s_memtime(); lds_barrier(); const uint64_t t2_ = __builtin_amdgcn_s_memtime(); \
                            clk_work += t1_ - clk_t; clk_wait += t2_ - t1_; clk_t = t2_; } while (0)
#define ROLE_CLK_DONE(slot) do { if (hi_ == 0 && lane == 0) { atomicAdd((unsigned long long *) (sc.err + 4) + 2 * (slot), (unsigned long long) clk_work); \
                                 atomicAdd((unsigned long long *) (sc.err + 4) + 2 * (slot) + 1, (unsigned long long) clk_wait); } } while (0)
#else
#define ROLE_CLK_INIT() do { } while (0)
#define ROLE_BARRIER() lds_barrier()
#define ROLE_CLK_DONE(slot) do { } while (0)
#endif

#ifdef PRUNE_EXP_CLOCK2 /* sections of the chain wave instead: kept merge cells, candidates, histogram + cutoff, selection, ties, next merge cells */
#define SEC_INIT() uint64_t sec_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; uint64_t sec_t = __builtin_amdgcn_s_memtime()
#define SEC_COUNT(i) do { sec_[i] += 1; } while (0) /* columns by path: 8 keep-all, 9 sorted, 10 histogram (one chunk), 11 histogram (several chunks) */
#define SEC(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); sec_[i] += t_ - sec_t; sec_t = t_; } while (0)
#define SEC_DONE() do { if (hi_ == 0 && lane == 0) for (int i_ = 0; i_ < 12; i_++) atomicAdd((unsigned long long *) (sc.err + 4) + i_, (unsigned long long) sec_[i_]); } while (0)
#else
#define SEC_INIT() do { } while (0)
#define SEC(i) do { } while (0)
#define SEC_COUNT(i) do { } while (0)
#define SEC_DONE() do { } while (0)
#endif

/* (PRUNE_SP, PRUNE_TAB and the size of the LDS layout below: mrp_level_order.h, prune_lds_bytes) */

/* T threads; the bin-streaming waves (all but the first four) form NGRP groups (2: alternating over the columns, a column's f and
 * b sit in a group's registers for two column times; 1: one group, requested one column ahead) and hold CPT loads of VEC cells
 * per lane and array. */
template <int T, int CPT, int NGRP, int VEC, bool PAIRS>
__global__ void __launch_bounds__(T, T <= 512 ? 4 : 1) mrp_prune_kernel(PruneIn d, const PruneHmm *__restrict__ hmms, int64_t n_hmms,
                                                      PruneParams p, PruneScratch sc) {
    constexpr int W = T / WAVE;
    constexpr int NBG = (W - 4) / NGRP;  /* waves per bin-streaming group; none (T = 256): columns of at most 64 CPT cells, whose
                                          * bins the table wave writes beside its tables -- four waves per workgroup, four
                                          * workgroups per CU where the register file allows two of eight waves */
    constexpr int LG = NBG > 0 ? NBG * WAVE : WAVE; /* lanes per group */
    static_assert((W == 4 || W >= 6) && ((W - 4) % NGRP) == 0 && (NGRP == 1 || NGRP == 2) && (VEC == 1 || VEC == 4), "role layout");
    extern __shared__ uint32_t lds[];
    const int S = p.S;
    const int nb = p.n_bins;
    const bool units = PAIRS && p.pairs == 2; /* the level's f, b and merge arrays hold one entry per unit (MRP_XF_UNITS) */
    const int nb_r = 1024; /* 16 bins per lane of the cutoff search: bin b lives at (b & 15) * 64 + (b >> 4) */
    /* posterior bins in LDS, two columns: one per cell; PAIRS: one per unit (cells 2u, 2u + 1 tie) */
    const int cap_c = PAIRS ? ((p.max_cells + 1) / 2 + 3) & ~3 : (p.max_cells + 3) & ~3;
    /* LDS layout (dwords) */
    uint32_t *sel = lds;                       /* [2][2][SP] selection of column k in buffer k & 1: key = bin << 14 | cell, np = next | prev << 16 */
    uint32_t *um = sel + 4 * PRUNE_SP;         /* [SP] posterior bin of the merge cell each selected cell leads to (selection order); wave 1 */
    uint32_t *s1 = um + PRUNE_SP;              /* [2][2][SP] stage 1 -> stage 2: next | prev and merge posterior bin per sorted kept cell */
    uint32_t *sh = s1 + 4 * PRUNE_SP;          /* [64] counters: n of the selection buffers at [32, 34), of the stage-1 buffers at [36, 38), of the kept merge lists at [40, 42) */
    uint32_t *hist = sh + 64;                  /* [2][nb_r] */
    uint32_t *bmp_c = hist + 2 * nb_r;         /* [512] cells of the cutoff bin, by cell index */
    uint32_t *bmp_m = bmp_c + 512;             /* [512] next merge cells seen */
    uint32_t *kml = bmp_m + 512;               /* [2][SP] kept merge cells leading into column k, buffer k & 1 */
    uint32_t *minfo = kml + 2 * PRUNE_SP;      /* [SP][2] per kept merge cell: what its candidates need (wave 0) */
    uint32_t *heads = minfo + 2 * PRUNE_SP;    /* [512] "a range starts here" marks of one chunk of candidates, zero between uses (wave 0) */
    uint32_t *pref = heads + 512;              /* [512] marks before each word of the cutoff bin's bitmap (wave 0) */
    uint32_t *tab = pref + 512;                /* [2 buffers][2 sides][PRUNE_TAB][128] */
    uint32_t *htab_key = tab + 4 * PRUNE_TAB * 128; /* [256] merge cell -> first kept cell that uses it (open addressing); wave 2 */
    uint32_t *htab_val = htab_key + 256;       /* [256] */
    uint32_t *flagw = htab_val + 256;          /* [max_merge bits] kept flag per merge cell (backward pass) */
    const int n_flagw = ((p.max_merge + 127) >> 7) << 2; /* words, a multiple of four */
    uint16_t *bins = reinterpret_cast<uint16_t *>(flagw + n_flagw); /* [2][cap_c] posterior bin per cell */
    auto flag_get = [&](uint32_t i) -> bool { return (flagw[i >> 5] >> (i & 31u)) & 1u; };
    auto flag_set = [&](uint32_t i) { atomicOr(&flagw[i >> 5], 1u << (i & 31u)); };
    auto flag_clr = [&](uint32_t i) { atomicAnd(&flagw[i >> 5], ~(1u << (i & 31u))); };

    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    /* The four role waves of a workgroup sit on the CU's four SIMDs (wave i on SIMD i mod 4).  Workgroups that share a CU
     * rotate the roles: otherwise every chain wave -- the one wave of a workgroup that is busy all the time -- would issue
     * from SIMD 0 and the workgroups would take turns on it. */
    const int hw_wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int wave = hw_wave < 4 ? ((hw_wave + (int) (blockIdx.x & 3u)) & 3) : hw_wave;
    const uint64_t lt_mask = (1ull << lane) - 1ull;

    for (int64_t hi_ = blockIdx.x; hi_ < n_hmms; hi_ += gridDim.x) {
        int errbits = 0;
        const PruneHmm h = k_load(hmms + hi_);
        const int K = h.n_cols;
        const int32_t total = (int32_t) d.hmm_fb[2 * h.hmm_index]; /* max mode: the same integer for every column */
        for (int i = tid; i < 2 * nb_r; i += T) hist[i] = 0;
        for (int i = tid; i < 1024; i += T) bmp_c[i] = 0; /* both bitmaps */
        for (int i = tid; i < 512; i += T) heads[i] = 0;
        for (int i = tid; i < n_flagw; i += T) flagw[i] = 0;
        if (tid < 64) sh[tid] = 0u;
        __syncthreads();

        /* The sorted lists of a finished selection, in two stages one column apart.  Nothing later in the forward pass
         * reads them: the next column's kept merge cells were already listed by wave 0 from the unsorted selection.
         * Stage 1 (wave 1, column kk from selection buffer kk & 1): stable sort of the kept cells, kept lists to HBM, the
         * posterior bins of the merge cells they lead to; leaves next | prev and that bin per sorted kept cell in LDS. */
        auto lists_stage1 = [&](int kk, int64_t mcell_off) {
            if constexpr (PAIRS) {
                /* Complement pairs (see the chain wave): the selection holds UNITS, at most 64; a unit's two cells tie and are
                 * neighbours in list order, so the sorted units, each expanded to (cell 2u, cell 2u + 1), are the sorted cells */
                const int b = kk & 1;
                const uint2 *selb = reinterpret_cast<const uint2 *>(sel) + b * 64; /* (bin << 14 | unit, next | prev << 16) */
                uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
                const int n = (int) sh[32 + b];
                const uint32_t fl = sh[44 + b]; /* bit 0: the column's cells come in pairs, 1: the merge cells after it, 2: those before it */
                const uint32_t o_pm = (fl >> 1) & 1u, i_pm = (fl >> 2) & 1u;
                const int64_t lcol = h.col0 + kk;
                const bool has_merge = kk + 1 < K;
                uint32_t key[1];
                int32_t pre_mf = 0, pre_mb = 0;
                const uint2 mine = selb[lane];
                key[0] = lane < n ? (mine.x << 7) | (uint32_t) lane : 0xFFFFFFFFu; /* bin (10) | unit (14) | slot (7) */
                if (has_merge && lane < n) {
                    const uint32_t m = mine.y & 0xFFFFu;
                    pre_mf = d.merge_f32[mcell_off + m];
                    pre_mb = d.merge_b32[mcell_off + m];
                }
                wave_bitonic_sort_n<1>(key, lane);
                if (has_merge) {
                    if (lane < n) um[lane] = (uint32_t) posterior_bin(pre_mf, pre_mb, total, nb, &errbits);
                    wave_lds_fence();
                }
                if (lane < n) {
                    const uint32_t src = key[0] & 0x7Fu, u = (key[0] >> 7) & 0x3FFFu, np_ = selb[src].y;
                    if (fl & 1u) {
                        *reinterpret_cast<uint32_t *>(sc.kept + lcol * S + 2 * lane) = (2u * u) | ((2u * u + 1u) << 16);
                        *reinterpret_cast<uint2 *>(sc.kept_np + lcol * S + 2 * lane) = make_uint2(np_, np_ ^ o_pm ^ (i_pm << 16));
                    } else { /* a column of one cell */
                        sc.kept[lcol * S + lane] = (uint16_t) u;
                        sc.kept_np[lcol * S + lane] = np_;
                    }
                    snp[lane] = np_;
                    if (has_merge) sbin[lane] = um[src];
                }
                if (lane == 0) { sc.n_kept[lcol] = (fl & 1u) ? 2 * n : n; sh[36 + b] = (uint32_t) n; sh[46 + b] = fl; }
                return;
            }
            const int b = kk & 1;
            const uint32_t *skey = sel + b * 2 * PRUNE_SP, *snp_in = skey + PRUNE_SP;
            uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
            const int n = (int) sh[32 + b];
            const int64_t lcol = h.col0 + kk;
            const bool has_merge = kk + 1 < K;
            uint32_t key[2];
            int32_t pre_mf[2] = {0, 0}, pre_mb[2] = {0, 0};
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int i = lane + u * WAVE;
                /* stable descending sort of the kept cells (stList_sort :1071): smaller bin = larger posterior, then list
                 * order = cell index; the slot rides along in the low bits: bin (10) | cell (14) | slot (7) */
                key[u] = i < n ? (skey[i] << 7) | (uint32_t) i : 0xFFFFFFFFu;
                /* the posteriors of the merge cells the selected cells lead to are requested now, for the selection in
                 * its unsorted order, and consumed after the sort */
                if (has_merge && i < n) {
                    const uint32_t m = snp_in[i] & 0xFFFFu;
                    pre_mf[u] = d.merge_f32[mcell_off + m];
                    pre_mb[u] = d.merge_b32[mcell_off + m];
                }
            }
            wave_bitonic_sort128(key[0], key[1], lane);
            if (has_merge) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int i = lane + u * WAVE;
                    if (i < n) um[i] = (uint32_t) posterior_bin(pre_mf[u], pre_mb[u], total, nb, &errbits);
                }
                wave_lds_fence();
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int i = lane + u * WAVE;
                if (i < n) {
                    const uint32_t src = key[u] & 0x7Fu, cell = (key[u] >> 7) & 0x3FFFu, np_ = snp_in[src];
                    sc.kept[lcol * S + i] = (uint16_t) cell;
                    sc.kept_np[lcol * S + i] = np_;
                    snp[i] = np_;
                    if (has_merge) sbin[i] = um[src];
                }
            }
            if (lane == 0) { sc.n_kept[lcol] = n; sh[36 + b] = (uint32_t) n; }
        };
        /* PAIRS: stage 1 in two halves a column apart -- the posteriors of the merge cells are a gather from HBM (two microseconds
         * under load, as long as a whole column of the chain on pairs): asked for when the selection of column kk is read (step
         * kk + 1), used a step later, with the selection in registers meanwhile (the chain reuses its buffer). */
        uint32_t p1_key = 0xFFFFFFFFu, p1_np = 0u, p1_fl = 0u;
        int32_t p1_mf = 0, p1_mb = 0;
        int p1_n = 0;
        auto stage1_ask = [&](int kk, int64_t mcell_off) {
            const int b = kk & 1;
            const uint2 *selb = reinterpret_cast<const uint2 *>(sel) + b * 64; /* (bin << 14 | unit, next | prev << 16) */
            p1_n = (int) sh[32 + b];
            p1_fl = sh[44 + b]; /* bit 0: the column's cells come in pairs, 1: the merge cells after it, 2: those before it */
            const uint2 mine = selb[lane];
            p1_key = lane < p1_n ? (mine.x << 7) | (uint32_t) lane : 0xFFFFFFFFu; /* bin (10) | unit (14) | slot (7) */
            p1_np = mine.y;
            p1_mf = 0; p1_mb = 0;
            if (kk + 1 < K && lane < p1_n) {
                const uint32_t m = (mine.y & 0xFFFFu) >> (units ? (p1_fl >> 1) & 1u : 0u); /* (units: the merge arrays hold merge units) */
                p1_mf = d.merge_f32[mcell_off + m];
                p1_mb = d.merge_b32[mcell_off + m];
            }
        };
        auto stage1_finish = [&](int kk) {
            const int b = kk & 1;
            uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
            const int n = p1_n;
            const uint32_t fl = p1_fl, o_pm = (fl >> 1) & 1u, i_pm = (fl >> 2) & 1u;
            const int64_t lcol = h.col0 + kk;
            const bool has_merge = kk + 1 < K;
            uint32_t key[1] = {p1_key};
            wave_bitonic_sort_n<1>(key, lane);
            const uint32_t mbin = has_merge && lane < n ? (uint32_t) posterior_bin(p1_mf, p1_mb, total, nb, &errbits) : 0u;
            /* what rides along with a unit comes from the lane that held it before the sort */
            const uint32_t src = key[0] & 0x3Fu, u = (key[0] >> 7) & 0x3FFFu;
            const uint32_t np_ = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (src << 2), (int) p1_np);
            const uint32_t sb_ = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (src << 2), (int) mbin);
            if (lane < n) {
                if (fl & 1u) {
                    *reinterpret_cast<uint32_t *>(sc.kept + lcol * S + 2 * lane) = (2u * u) | ((2u * u + 1u) << 16);
                    *reinterpret_cast<uint2 *>(sc.kept_np + lcol * S + 2 * lane) = make_uint2(np_, np_ ^ o_pm ^ (i_pm << 16));
                } else { /* a column of one cell */
                    sc.kept[lcol * S + lane] = (uint16_t) u;
                    sc.kept_np[lcol * S + lane] = np_;
                }
                snp[lane] = np_;
                sbin[lane] = sb_;
            }
            if (lane == 0) { sc.n_kept[lcol] = (fl & 1u) ? 2 * n : n; sh[36 + b] = (uint32_t) n; sh[46 + b] = fl; }
        };
        /* Stage 2 (wave 2, one column later): distinct next merge cells in order of first use, stable sort by posterior,
         * kept merge list to HBM. */
        auto lists_stage2 = [&](int kk) {
            if constexpr (PAIRS) {
                const int b = kk & 1;
                const uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
                const int n = (int) sh[36 + b];
                const uint32_t o_pm = (sh[46 + b] >> 1) & 1u;
                const int64_t lcol = h.col0 + kk;
                int mn_out = 0;
                if (kk + 1 < K) {
                    /* distinct next merge UNITS in order of first use; the two merge cells of a unit enter the list in the order the
                     * unit's first user reaches them: its even cell first (bit q of that cell's merge cell index), then its twin */
                    for (int i = lane; i < 256; i += WAVE) { htab_key[i] = 0xFFFFFFFFu; htab_val[i] = 0xFFFFFFFFu; }
                    wave_lds_fence();
                    uint32_t my_mu = 0u, my_q = 0u;
                    int slot = 0;
                    if (lane < n) {
                        const uint32_t mfull = snp[lane] & 0xFFFFu;
                        my_mu = mfull >> o_pm; my_q = mfull & o_pm;
                        int q = (int) ((my_mu * 2654435761u) >> 24);
                        for (;;) {
                            const uint32_t prev = atomicCAS(&htab_key[q], 0xFFFFFFFFu, my_mu);
                            if (prev == 0xFFFFFFFFu || prev == my_mu) break;
                            q = (q + 1) & 255;
                        }
                        slot = q;
                        atomicMin(&htab_val[q], (uint32_t) lane);
                    }
                    wave_lds_fence();
                    const bool first = lane < n && htab_val[slot] == (uint32_t) lane;
                    const uint64_t f0 = __ballot(first);
                    const int mnl = __popcll(f0);
                    uint32_t mkey[1] = {0xFFFFFFFFu};
                    bool pass_thr = false;
                    if (first) {
                        const int pos = (int) lanemask_lt_count(f0, lane);
                        const int bin = (int) sbin[lane];
                        pass_thr = bin <= p.thr_bin;
                        mkey[0] = ((uint32_t) bin << 20) | ((uint32_t) pos << 14) | (my_mu << 1) | my_q;
                    }
                    const int gm = __popcll(__ballot(pass_thr));
                    const int wm = o_pm ? 2 : 1;
                    const int mn = kept_count(mnl * wm, gm * wm, p.min_p, p.max_p);
                    if (mn != mnl * wm || (p.pad && hi_ == 0 && kk == 0)) errbits |= MRP_ENGINE_ERR_MERGE;
                    wave_bitonic_sort_n<1>(mkey, lane);
                    if (lane < mnl) {
                        const uint32_t mu = (mkey[0] >> 1) & 0x1FFFu, q = mkey[0] & 1u;
                        if (o_pm) *reinterpret_cast<uint32_t *>(sc.keptm + lcol * S + 2 * lane) = (2u * mu + q) | ((2u * mu + (q ^ 1u)) << 16);
                        else sc.keptm[lcol * S + lane] = (uint16_t) mu;
                    }
                    mn_out = mnl * wm;
                }
                if (lane == 0) sc.n_keptm[lcol] = mn_out;
                return;
            }
            const int b = kk & 1;
            const uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
            const int n = (int) sh[36 + b];
            const int64_t lcol = h.col0 + kk;
            int mn = 0;
            if (kk + 1 < K) {
                /* getLinkedMergeCells :989-1004: distinct next merge cells in order of first use (sorted order of the
                 * kept cells): a 256-slot open-addressing table, merge cell -> smallest sorted index that uses it */
                for (int i = lane; i < 256; i += WAVE) { htab_key[i] = 0xFFFFFFFFu; htab_val[i] = 0xFFFFFFFFu; }
                wave_lds_fence();
                uint32_t my_m[2] = {0u, 0u};
                int slot[2] = {0, 0};
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int i = lane + u * WAVE;
                    if (i < n) {
                        const uint32_t m = snp[i] & 0xFFFFu;
                        my_m[u] = m;
                        int q = (int) ((m * 2654435761u) >> 24);
                        for (;;) {
                            const uint32_t prev = atomicCAS(&htab_key[q], 0xFFFFFFFFu, m);
                            if (prev == 0xFFFFFFFFu || prev == m) break;
                            q = (q + 1) & 255;
                        }
                        slot[u] = q;
                        atomicMin(&htab_val[q], (uint32_t) i);
                    }
                }
                wave_lds_fence();
                bool first[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int i = lane + u * WAVE;
                    first[u] = i < n && htab_val[slot[u]] == (uint32_t) i;
                }
                const uint64_t f0 = __ballot(first[0]), f1 = __ballot(first[1]);
                const int mnl = __popcll(f0) + __popcll(f1);
                uint32_t mkey[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
                int pass_thr[2] = {0, 0};
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (first[u]) {
                        const int pos = u == 0 ? (int) lanemask_lt_count(f0, lane) : __popcll(f0) + (int) lanemask_lt_count(f1, lane);
                        const int bin = (int) sbin[lane + u * WAVE];
                        pass_thr[u] = bin <= p.thr_bin ? 1 : 0;
                        mkey[u] = ((uint32_t) bin << 21) | ((uint32_t) pos << 14) | my_m[u];
                    }
                }
                const int gm = __popcll(__ballot(pass_thr[0] != 0)) + __popcll(__ballot(pass_thr[1] != 0));
                mn = kept_count(mnl, gm, p.min_p, p.max_p);
                /* Wave 0 has kept EVERY distinct next merge cell.  That is what :1090-1100 keeps: a merge cell's
                 * posterior is at least that of any cell leading to it (max mode, exact integers), so whenever more
                 * than min_p cells were kept they all pass the threshold, and so do their merge cells.  Checked, not
                 * assumed: a violation discards the hmm (the host redoes its chunk on the hashing path). */
                if (mn != mnl || (p.pad && hi_ == 0 && kk == 0)) errbits |= MRP_ENGINE_ERR_MERGE; /* p.pad: fault injection of the tests */
                /* stable descending sort by posterior (:1090) */
                wave_bitonic_sort128(mkey[0], mkey[1], lane);
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int r = lane + u * WAVE;
                    if (r < mn) sc.keptm[lcol * S + r] = (uint16_t) (mkey[u] & 0x3FFFu);
                }
            }
            if (lane == 0) sc.n_keptm[lcol] = mn;
        };

        /* ---- stRPHmm_pruneForwards hmm.c:1049-1109 ----
         * Every role runs its own loop over the columns (the registers of one role are not live in the others); all of them
         * pass the same barriers: one after the prologue, one per column, one before the last merge list. */
        if (wave == 0) {
            /* the chain wave goes first whenever it can issue: alone on the device that changes nothing (its SIMD's helper
             * waves are parked), beside the kernels of other batches on the same CU it is worth ~2 % of a call */
            __builtin_amdgcn_s_setprio(3);
            if (lane == 0) {
                kml[0] = 0u;   /* column 0: every cell is "linked" (one virtual merge cell in front of it) */
                sh[40] = 1u;
            }
            lds_barrier();
            ROLE_CLK_INIT();
            SEC_INIT();
            if constexpr (PAIRS) {
            /* ---- the chain on complement PAIRS (includeInvertedPartitions, even column limits) ----
             * Every cell of a cross product column has its complement next to it (cells 2u, 2u + 1 = "unit" u; the order rule of
             * cross_cell / pair_index), with the same cost, f, b and posterior, and the twin's merge cells are the twins of its
             * merge cells.  A kept merge cell is kept with its twin, linked cells are linked with their twins, ties between twins
             * fall in list order (2u before 2u + 1), and the limits are even, so the forward pass never separates a pair: the
             * chain carries UNITS -- half the kept merge cells (one per lane), half the candidates, half the selection -- and waves
             * 1 and 2 write both cells of every kept unit.  A unit is named by ANY of its two members where that is cheaper:
             *   unit(x, y)   = (x >> 1) * Y + ((y ^ (x & xm)) >> sb)      x, y: indices on side A / B, Y: side B's count
             *   parity(x, y) = (x & pa) | (y & sb)                         which member of its unit the pair (x, y) is
             * with xm = both sides paired, sb = only side B paired, pa = side A paired (all wave-uniform).  A column or merge
             * column with neither side paired has one self-complementary entry: a unit of one cell.  The cells linked to ONE
             * member of a kept merge unit are one member of every linked unit, so the enumeration is that of the general
             * kernel over half the entries; only behind a merge column of one cell both members turn up, and the odd ones are
             * dropped. */
            /* One slot of 64 candidates at a time, start to finish (owner, parent cells, unit, posterior bin, next merge unit):
             * the slots of a column are independent, but a column links 65 units on average -- one or two slots -- and code that
             * keeps eight slots in flight at once spends more instructions moving its register tuples through the "has this slot
             * work" branches than on the work.  Records of the kept merge units (16 bytes, with the reciprocal for the division
             * by the side-B count), the selection (key and transitions as one 8-byte entry) and the marks sit in LDS. */
            uint4 *rec = reinterpret_cast<uint4 *>(minfo);       /* [64] per kept merge unit of the column */
            for (int k = 0; k < K; k++) {
                SEC(7);
                const int b = k & 1;
                const uint4 cd = *reinterpret_cast<const uint4 *>(sh + 48 + 4 * b);
                const int nkm = (int) sh[40 + b];
                const uint32_t ent_ = kml[b * PRUNE_SP + lane];
                const uint32_t cd0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.x), cd1 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.y);
                const uint32_t cd2 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.z); /* the table wave's bits */
                uint2 *selb = reinterpret_cast<uint2 *>(sel) + b * 64; /* selection of column k: (bin << 14 | unit, next | prev << 16 of the unit's even cell) */
                const uint32_t *tA = tab + b * 2 * PRUNE_TAB * 128, *tB = tA + PRUNE_TAB * 128;
                const uint32_t *csA = tA + 128, *listA = tA + 256, *nxA = tA + 384;
                const uint32_t *csB = tB + 128, *listB = tB + 256, *nxB = tB + 384;
                const uint16_t *bin_k = bins + b * cap_c;
                uint32_t *hk = hist + b * nb_r;
                uint32_t *kmn = kml + (b ^ 1) * PRUNE_SP; /* the kept merge units leading into column k + 1 */
                const uint32_t cflags = cd1 & 0xFFu;
                const uint32_t C2 = (cd0 & 0xFFFFu) > 128u ? 128u : (cd0 & 0xFFFFu), Mb = cd0 >> 16, Pb = cd1 >> 16;
                const bool a_cp = (cd1 & 0x100u) != 0, b_cp = (cd1 & 0x200u) != 0;
                const bool in_ap = (cflags & MRP_XF_IN_A_PAIRED) != 0, in_bp = (cflags & MRP_XF_IN_B_PAIRED) != 0;
                const bool has_next = k + 1 < K;
                const uint32_t c_xm = cd2 & 1u, c_sb = (cd2 >> 1) & 1u, c_pa = (cd2 >> 2) & 1u;
                const uint32_t o_xm = (cd2 >> 3) & 1u, o_sb = (cd2 >> 4) & 1u, o_pa = (cd2 >> 5) & 1u;
                const uint32_t o_pm = (cd2 >> 6) & 1u, i_pm = (cd2 >> 7) & 1u;
                const uint32_t i_pa = (cd2 >> 8) & 1u, i_sb = (cd2 >> 9) & 1u;
                const int w_sh = (int) ((cd2 >> 10) & 1u), w_c = 1 << w_sh;  /* cells per unit of this column: 1 << w_sh */
                const bool filt = ((cd2 >> 11) & 1u) != 0;  /* behind a merge column of one cell: both members are enumerated */
                /* this lane's kept merge unit: the parents' cells one of its members links, as list ranges.  An entry of the
                 * list is unit | i << 14 | j << 21: the unit and the indices of that member on either side */
                const bool has = lane < nkm;
                const uint32_t ent = has ? ent_ : 0u;
                const uint32_t e_i = (ent >> 14) & 127u, e_j = (ent >> 21) & 127u;
                const uint32_t e_csa = csA[e_i], e_csb = csB[e_j]; /* first entry | size << 8 of the group in the inverted lists */
                const uint32_t e_nb = has ? e_csb >> 8 : 0u;
                const int tot = has ? (int) ((e_csa >> 8) * e_nb) : 0;
                if (has && tot == 0) errbits |= MRP_ENGINE_ERR_RANGE; /* (a kept merge cell links at least one cell: the owners below count on it) */
                const int incl = wave_incl_scan_bc(tot);
                const int L = __builtin_amdgcn_readlane(incl, WAVE - 1); /* pairs of parent cells enumerated */
                const int off = incl - tot;
                {
                    const uint32_t e_par = (e_i & i_pa) | (e_j & i_sb);     /* which member of its unit the entry names */
                    const float rn = __builtin_amdgcn_rcpf((float) (e_nb ? e_nb : 1u));
                    if (has) rec[lane] = make_uint4((ent & 0x3FFFu) | (e_nb << 14) | (e_par << 22), (uint32_t) off | ((e_csa & 0xFFu) << 14) | ((e_csb & 0xFFu) << 21),
                                                    __float_as_uint(rn), 0u);
                }
                const int Lu = filt ? L >> 1 : L;  /* linked units */
                const int Lc = Lu << w_sh;         /* linked cells */
                SEC(0);
                const bool thr_all = p.thr_bin >= nb - 1;
                const bool keep_all = Lc <= p.min_p || (thr_all && Lc <= p.max_p); /* the loop of :1073-1079 drops nothing */
                auto kept_units = [&](int g_units) -> int { return kept_count(Lc, g_units << w_sh, p.min_p, p.max_p) >> w_sh; };
                /* candidates q0 .. q0 + 63: key = bin << 14 | unit (0xFFFFFFFF: none), the parent cells the enumeration met, and the
                 * merge cell the unit's EVEN cell comes from */
                auto slot = [&](int q0, uint32_t &c1, uint32_t &c2, uint32_t &prv_even) -> uint32_t {
                    /* marks: index + 1 of the kept merge unit whose range starts (or, at position 0, continues) here.  The
                     * ranges follow each other without gaps, so the owner of a position is the first owner plus the marks
                     * up to it: no prefix maximum */
                    if (tot > 0 && off + tot > q0 && off < q0 + WAVE) heads[off > q0 ? off - q0 : 0] = (uint32_t) lane + 1u;
                    wave_lds_fence();
                    const uint32_t own = heads[lane];
                    heads[lane] = 0u; /* left clean for the next use */
                    const uint64_t marks = __ballot(own != 0u);
                    const int first_owner = __builtin_amdgcn_readfirstlane((int) own) - 1;
                    const int owner = first_owner + mbcnt64(marks) + (own != 0u ? 1 : 0) - 1;
                    const bool in = q0 + lane < L;
                    const uint4 r = rec[in ? owner & 63 : 0];
                    const uint32_t nbq = (r.x >> 14) & 0xFFu, sa = (r.y >> 14) & 0x7Fu, sb = (r.y >> 21) & 0x7Fu;
                    const uint32_t t = (uint32_t) (q0 + lane) - (r.y & 0x3FFFu);
                    /* t = x * nb + y: (t + 0.5) / nb is at least 0.5 / nb away from an integer and the float product is off by less */
                    const uint32_t x = (uint32_t) (((float) t + 0.5f) * __uint_as_float(r.z));
                    const uint32_t y = t - x * nbq;
                    c1 = listA[(sa + x) & 127u];
                    c2 = listB[(sb + y) & 127u];
                    const uint32_t par_c = (c1 & c_pa) | (c2 & c_sb);
                    const uint32_t u = in ? (c1 >> 1) * C2 + ((c2 ^ (c1 & c_xm)) >> c_sb) : 0u;
                    prv_even = ((r.x & 0x3FFFu) << 1) + ((((r.x >> 22) & 1u) ^ par_c) & i_pm);
                    const uint32_t bin_ = bin_k[u];
                    return (!in || (filt && par_c != 0u)) ? 0xFFFFFFFFu : ((bin_ << 14) | u);
                };
                /* a selected candidate: its slot of the selection, and -- the first time its next merge unit is seen -- that unit as
                 * a kept merge unit of the next column.  Called in wave-uniform control flow, `take` per lane. */
                int cm = 0;
                auto emit = [&](bool take, int pos, uint32_t key_, uint32_t c1, uint32_t c2, uint32_t prv_even) {
                    const uint32_t ii = nxA[c1 & 127u], jj = nxB[c2 & 127u];
                    const uint32_t par_c = (c1 & c_pa) | (c2 & c_sb);
                    const uint32_t mu2 = has_next ? (ii >> 1) * Mb + ((jj ^ (ii & o_xm)) >> o_sb) : 0u;
                    const uint32_t par_m = (ii & o_pa) | (jj & o_sb);
                    const uint32_t nxt_even = (mu2 << 1) + ((par_m ^ par_c) & o_pm); /* the merge cell the unit's EVEN cell leads to */
                    if (take) selb[pos & 63] = make_uint2(key_, nxt_even | (prv_even << 16));
                    if (has_next) {
                        bool first = false;
                        if (take) {
                            const uint32_t bit = 1u << (mu2 & 31u);
                            first = (atomicOr(&bmp_m[(mu2 >> 5) & 511u], bit) & bit) == 0u;
                        }
                        const uint64_t fm = __ballot(first);
                        if (first) kmn[(cm + mbcnt64(fm)) & 127] = mu2 | (ii << 14) | (jj << 21);
                        cm += __popcll(fm);
                    }
                };
                int n = 0;
                /* Columns of up to 64 NS candidates (NS = 1, 2, 4: nine columns in ten): the NS slots side by side in straight-line
                 * code -- one fence for all their marks, their LDS round trips overlapped -- then either every candidate is kept
                 * (emit in enumeration order; the list stage sorts) or the kept units are the first n of the sorted keys. */
                auto small_col = [&](auto ns_tag) {
                    constexpr int NS = decltype(ns_tag)::value;
                    if (tot > 0) { /* marks: where this unit's range starts, and the slots it continues into */
                        if (off < NS * WAVE) heads[off] = (uint32_t) lane + 1u;
#pragma unroll
                        for (int j = 1; j < NS; j++)
                            if (off < j * WAVE && off + tot > j * WAVE) heads[j * WAVE] = (uint32_t) lane + 1u;
                    }
                    wave_lds_fence();
                    uint32_t own[NS], key[NS], c1[NS], c2[NS], pe[NS];
#pragma unroll
                    for (int j = 0; j < NS; j++) { own[j] = heads[j * WAVE + lane]; heads[j * WAVE + lane] = 0u; }
                    uint4 r[NS];
                    bool in[NS];
#pragma unroll
                    for (int j = 0; j < NS; j++) {
                        const uint64_t marks = __ballot(own[j] != 0u);
                        const int first_owner = __builtin_amdgcn_readfirstlane((int) own[j]) - 1;
                        const int owner = first_owner + mbcnt64(marks) + (own[j] != 0u ? 1 : 0) - 1;
                        in[j] = j * WAVE + lane < L;
                        r[j] = rec[in[j] ? owner & 63 : 0];
                    }
#pragma unroll
                    for (int j = 0; j < NS; j++) {
                        const uint32_t nbq = (r[j].x >> 14) & 0xFFu, sa = (r[j].y >> 14) & 0x7Fu, sb = (r[j].y >> 21) & 0x7Fu;
                        const uint32_t t = (uint32_t) (j * WAVE + lane) - (r[j].y & 0x3FFFu);
                        const uint32_t x = (uint32_t) (((float) t + 0.5f) * __uint_as_float(r[j].z)); /* exact: see slot() */
                        const uint32_t y = t - x * nbq;
                        c1[j] = listA[(sa + x) & 127u];
                        c2[j] = listB[(sb + y) & 127u];
                    }
                    uint32_t ii[NS], jj[NS];
#pragma unroll
                    for (int j = 0; j < NS; j++) {
                        const uint32_t par_c = (c1[j] & c_pa) | (c2[j] & c_sb);
                        const uint32_t u = in[j] ? (c1[j] >> 1) * C2 + ((c2[j] ^ (c1[j] & c_xm)) >> c_sb) : 0u;
                        pe[j] = ((r[j].x & 0x3FFFu) << 1) + ((((r[j].x >> 22) & 1u) ^ par_c) & i_pm);
                        const uint32_t bin_ = bin_k[u];
                        if (keep_all) { ii[j] = nxA[c1[j] & 127u]; jj[j] = nxB[c2[j] & 127u]; } /* (wave-uniform: asked for together with the bins) */
                        key[j] = (!in[j] || (filt && par_c != 0u)) ? 0xFFFFFFFFu : ((bin_ << 14) | u);
                    }
                    if (keep_all) {
                        SEC_COUNT(8);
                        uint32_t mu2[NS], ent2[NS], old[NS];
#pragma unroll
                        for (int j = 0; j < NS; j++) {
                            const bool take = key[j] != 0xFFFFFFFFu;
                            const uint32_t par_c = (c1[j] & c_pa) | (c2[j] & c_sb);
                            mu2[j] = has_next ? (ii[j] >> 1) * Mb + ((jj[j] ^ (ii[j] & o_xm)) >> o_sb) : 0u;
                            const uint32_t par_m = (ii[j] & o_pa) | (jj[j] & o_sb);
                            const uint32_t nxt_even = (mu2[j] << 1) + ((par_m ^ par_c) & o_pm);
                            ent2[j] = mu2[j] | (ii[j] << 14) | (jj[j] << 21);
                            const uint64_t am = __ballot(take);
                            if (take) selb[(n + mbcnt64(am)) & 63] = make_uint2(key[j], nxt_even | (pe[j] << 16));
                            n += __popcll(am);
                            old[j] = 0xFFFFFFFFu;
                            if (has_next && take) old[j] = atomicOr(&bmp_m[(mu2[j] >> 5) & 511u], 1u << (mu2[j] & 31u));
                        }
                        if (has_next) {
#pragma unroll
                            for (int j = 0; j < NS; j++) {
                                const bool first = ((old[j] >> (mu2[j] & 31u)) & 1u) == 0u;
                                const uint64_t fm = __ballot(first);
                                if (first) kmn[(cm + mbcnt64(fm)) & 127] = ent2[j];
                                cm += __popcll(fm);
                            }
                        }
                        SEC(1);
                    } else {
                        SEC_COUNT(9);
                        int g = Lu;
                        if (!thr_all) {
                            g = 0;
#pragma unroll
                            for (int j = 0; j < NS; j++) g += __popcll(__ballot(key[j] != 0xFFFFFFFFu && (int) (key[j] >> 14) <= p.thr_bin));
                        }
                        n = kept_units(g);
                        wave_bitonic_sort_n<NS>(key, lane);
                        const uint32_t *pvA = tA + 512, *pvB = tB + 512;
                        /* n <= 64 units: the kept ones are in the first register.  The even cell of unit u and where it comes from: */
                        const bool take = lane < n;
                        const uint32_t u = take ? key[0] & 0x3FFFu : 0u;
                        uint32_t d1, d2;
                        if (a_cp) {
                            const uint32_t q = (uint32_t) (((float) u + 0.5f) * __builtin_amdgcn_rcpf((float) (C2 ? C2 : 1u)));
                            d1 = 2u * q; d2 = u - q * C2;
                        } else if (b_cp) { d1 = 0u; d2 = 2u * u; }
                        else { d1 = 0u; d2 = 0u; }
                        d1 &= 127u; d2 &= 127u;
                        const uint32_t prv = k > 0 ? pair_index(pvA[d1], pvB[d2], Pb, true, in_ap, in_bp) : 0u;
                        emit(take, lane, key[0], d1, d2, prv);
                        SEC(4);
                    }
                };
                if (L <= WAVE) small_col(std::integral_constant<int, 1>());
                else if (L <= 2 * WAVE) small_col(std::integral_constant<int, 2>());
                else if (L <= 4 * WAVE) small_col(std::integral_constant<int, 4>());
                else if (keep_all) {
                    SEC_COUNT(8);
#pragma unroll 1
                    for (int q0 = 0; q0 < L; q0 += WAVE) {
                        uint32_t c1, c2, pe;
                        const uint32_t key_ = slot(q0, c1, c2, pe);
                        const uint64_t am = __ballot(key_ != 0xFFFFFFFFu);
                        emit(key_ != 0xFFFFFFFFu, n + mbcnt64(am), key_, c1, c2, pe);
                        n += __popcll(am);
                    }
                    SEC(1);
                } else {
                    /* pass 1: histogram of the posterior bins */
                    if (lane == 0) sh[56 + b] = 1u; /* the table wave wipes this histogram before its next use */
                    SEC_COUNT(L > 512 ? 11 : 10);
#pragma unroll 1
                    for (int q0 = 0; q0 < L; q0 += WAVE) {
                        uint32_t c1, c2, pe;
                        const uint32_t key_ = slot(q0, c1, c2, pe);
                        if (key_ != 0xFFFFFFFFu) {
                            const int bin_ = (int) (key_ >> 14);
                            atomicAdd(&hk[(bin_ & 15) * WAVE + (bin_ >> 4)], 1u);
                        }
                    }
                    wave_lds_fence();
                    SEC(2);
                    /* cutoff bin and quota: lane l owns the 16 consecutive bins [16 l, 16 l + 16) */
                    int v[16];
                    int tot_l = 0, pass = 0;
                    const int thr_rel = p.thr_bin - lane * 16; /* bins q <= thr_rel of this lane pass the threshold */
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        v[q] = (int) hk[q * WAVE + lane];
                        tot_l += v[q];
                        if (q <= thr_rel) pass += v[q];
                    }
                    const int incl_h = wave_incl_scan(tot_l, lane);
                    const int g = thr_all ? Lu : __builtin_amdgcn_readlane(wave_incl_scan(pass, lane), WAVE - 1);
                    n = kept_units(g);
                    const int ex = incl_h - tot_l;
                    int myq = -1, myQ = 0, myV = 0;
                    const bool owner_lane = n > 0 && ex < n && n <= incl_h;
                    if (owner_lane) {
                        int cum = ex;
#pragma unroll
                        for (int q = 0; q < 16; q++) {
                            if (myq < 0 && cum + v[q] >= n) { myq = q; myQ = n - cum; myV = v[q]; }
                            cum += v[q];
                        }
                    }
                    const int myB = lane * 16 + myq;
                    const uint64_t om = __ballot(owner_lane);
                    const int srcu = __builtin_amdgcn_readfirstlane(om ? __ffsll((unsigned long long) om) - 1 : 0);
                    const int B = om ? __builtin_amdgcn_readlane(myB, srcu) : -1;
                    const int quota = om ? __builtin_amdgcn_readlane(myQ, srcu) : 0;
                    const int in_B = om ? __builtin_amdgcn_readlane(myV, srcu) : 0;
                    const int nG = n - quota;
                    const bool whole_bin = in_B == quota; /* the cutoff bin is kept entirely: no ranking needed */
                    SEC(3);
                    /* pass 2: the units above the cutoff bin; those in it are kept directly or marked by unit index */
                    int gc = 0, ec = 0;
#pragma unroll 1
                    for (int q0 = 0; q0 < L; q0 += WAVE) {
                        uint32_t c1, c2, pe;
                        const uint32_t key_ = slot(q0, c1, c2, pe);
                        const int bin_ = key_ != 0xFFFFFFFFu ? (int) (key_ >> 14) : nb;
                        const bool is_g = bin_ < B, is_e = bin_ == B;
                        const uint64_t mg = __ballot(is_g), me = __ballot(is_e);
                        const bool take = is_g || (is_e && whole_bin);
                        emit(take, is_g ? gc + mbcnt64(mg) : nG + ec + mbcnt64(me), key_, c1, c2, pe);
                        if (is_e && !whole_bin) {
                            const uint32_t e = key_ & 0x3FFFu;
                            atomicOr(&bmp_c[e >> 5], 1u << (e & 31u));
                        }
                        gc += __popcll(mg);
                        ec += __popcll(me);
                    }
                    SEC(4);
                    if (!whole_bin && quota > 0) {
                        /* the first `quota` units of the cutoff bin in list order (= by unit index): a unit's rank is the number
                         * of marks below it */
                        wave_lds_fence();
                        {
                            uint32_t w[8];
                            int cnt_l = 0;
#pragma unroll
                            for (int q = 0; q < 8; q++) { w[q] = bmp_c[lane * 8 + q]; cnt_l += __popc(w[q]); }
                            int run = wave_incl_scan(cnt_l, lane) - cnt_l;
#pragma unroll
                            for (int q = 0; q < 8; q++) { pref[lane * 8 + q] = (uint32_t) run; run += __popc(w[q]); }
                        }
                        wave_lds_fence();
#pragma unroll 1
                        for (int q0 = 0; q0 < L; q0 += WAVE) {
                            uint32_t c1, c2, pe;
                            const uint32_t key_ = slot(q0, c1, c2, pe);
                            const bool is_e = key_ != 0xFFFFFFFFu && (int) (key_ >> 14) == B;
                            const uint32_t e = key_ & 0x3FFFu, wd = is_e ? e >> 5 : 0u;
                            const int rank = (int) pref[wd] + __popc(bmp_c[wd] & ((1u << (e & 31u)) - 1u));
                            emit(is_e && rank < quota, nG + rank, key_, c1, c2, pe);
                        }
                        wave_lds_fence();
#pragma unroll 1
                        for (int q0 = 0; q0 < L; q0 += WAVE) { /* the marks go */
                            uint32_t c1, c2, pe;
                            const uint32_t key_ = slot(q0, c1, c2, pe);
                            if (key_ != 0xFFFFFFFFu && (int) (key_ >> 14) == B) bmp_c[(key_ & 0x3FFFu) >> 5] = 0u;
                        }
                    }
                }
                wave_lds_fence();
                SEC(5);
                if (lane == 0) {
                    sh[32 + b] = (uint32_t) n; sh[40 + (b ^ 1)] = (uint32_t) cm;
                    sh[44 + b] = (w_c == 2 ? 1u : 0u) | (o_pm << 1) | (i_pm << 2); /* for the list stages */
                }
                /* the marks of the next merge units go */
                if (has_next && lane < cm) bmp_m[((kmn[lane] & 0x3FFFu) >> 5) & 511u] = 0u;
                SEC(6);
                ROLE_BARRIER();
            }
            } else {
            for (int k = 0; k < K; k++) {
                SEC(7);
                /* the descriptor of the column after next: requested first, so that its latency hides behind this column's work
                 * (a scalar load issued just before the barrier would be waited for there: the barrier drains lgkmcnt) */
                const int b = k & 1;
                /* what the chain needs of the column's CrossCol comes through LDS from the table wave (sh[48 + 2 b ..]): a scalar
                 * load here would sit in the same counter as the LDS traffic, and every LDS wait of the column would wait for it */
                const uint32_t cd0 = sh[48 + 4 * b], cd1 = sh[49 + 4 * b];
                uint32_t *skey = sel + b * 2 * PRUNE_SP, *snp = skey + PRUNE_SP;
                const uint32_t *tA = tab + b * 2 * PRUNE_TAB * 128, *tB = tA + PRUNE_TAB * 128;
                const uint32_t *cntA = tA, *startA = tA + 128, *listA = tA + 256, *nxA = tA + 384;
                const uint32_t *cntB = tB, *startB = tB + 128, *listB = tB + 256, *nxB = tB + 384;
                const uint16_t *bin_k = bins + b * cap_c;
                uint32_t *hk = hist + b * nb_r;
                uint32_t *kmn = kml + (b ^ 1) * PRUNE_SP; /* the kept merge cells leading into column k + 1 */
                const uint32_t cflags = cd1 & 0xFFu;
                const bool inv = (cflags & MRP_XF_INVERTED) != 0;
                const uint32_t C2 = (cd0 & 0xFFFFu) > 128u ? 128u : (cd0 & 0xFFFFu), Mb = cd0 >> 16;
                const bool a_cp = inv && (cd1 & 0x100u), b_cp = inv && (cd1 & 0x200u);
                const bool out_ap = (cflags & MRP_XF_OUT_A_PAIRED) != 0, out_bp = (cflags & MRP_XF_OUT_B_PAIRED) != 0;
                const bool has_next = k + 1 < K;
                const int nkm = (int) sh[40 + b];
                /* this lane's kept merge cells (two at most): the parents' cells each links, as list ranges.  An entry of the
                 * list is m | i << 14 | j << 21: the merge cell and its index on either side (what links the parents' cells) */
                uint32_t off_[2];
                int tot[2];
                {
                    uint32_t m_[2], sa[2], sb_[2];
                    int nbb[2];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int idx = lane + u * WAVE;
                        const bool has = idx < nkm;
                        const uint32_t ent = has ? kml[b * PRUNE_SP + idx] : 0u;
                        m_[u] = ent & 0x3FFFu;
                        const uint32_t i = (ent >> 14) & 127u, j = (ent >> 21) & 127u;
                        sa[u] = startA[i]; sb_[u] = startB[j];
                        const int na = has ? (int) cntA[i] : 0;
                        nbb[u] = has ? (int) cntB[j] : 0;
                        tot[u] = na * nbb[u];
                    }
                    /* candidate q of the column belongs to the kept merge cell whose range [off, off + tot) holds it: ranges in
                     * list order of the kept merge cells (first all of this wave's "u = 0" entries, then the "u = 1" ones) */
                    const int i0 = wave_incl_scan(tot[0], lane);
                    const int t0 = __builtin_amdgcn_readlane(i0, WAVE - 1);
                    off_[0] = (uint32_t) (i0 - tot[0]);
                    off_[1] = (uint32_t) t0;
                    if (nkm > WAVE) {
                        const int i1 = wave_incl_scan(tot[1], lane);
                        off_[1] = (uint32_t) (t0 + i1 - tot[1]);
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) { /* what a candidate needs of its kept merge cell: two dwords */
                        const int idx = lane + u * WAVE;
                        if (idx < nkm) *reinterpret_cast<uint2 *>(minfo + 2 * idx) = make_uint2(m_[u] | ((uint32_t) nbb[u] << 14), off_[u] | (sa[u] << 14) | (sb_[u] << 21));
                    }
                }
                int L;
                {
                    const int l0 = wave_incl_scan(tot[0] + tot[1], lane);
                    L = __builtin_amdgcn_readlane(l0, WAVE - 1);
                }
                SEC(0);
                const bool thr_all = p.thr_bin >= nb - 1;
                const bool keep_all = L <= p.min_p || (thr_all && L <= p.max_p); /* the loop of :1073-1079 drops nothing */
                /* One chunk = up to 512 consecutive candidates in eight slots of 64 (slot j, lane l: candidate q0 + 64 j + l);
                 * only the ns slots the chunk needs are worked on (a column links 130 cells on average: two or three slots).
                 * Per slot: the owner (the kept merge cell whose range holds the candidate) by a prefix maximum over "a range
                 * starts here" marks, the owner's record, the two parent cells from the inverted lists, the cell index by
                 * the closed form of the cross product order, its posterior bin.  The slots' chains are independent. */
                uint32_t key[8], aux[8]; /* bin << 14 | cell (0xFFFFFFFF: none);  c1 | c2 << 8 | prev merge cell << 16 */
                auto load_chunk = [&](int q0) -> int {
                    const int left = L - q0;
                    const int ns = left >= 512 ? 8 : (left + 63) >> 6;
#pragma unroll
                    for (int u = 0; u < 2; u++) { /* marks: index + 1 of the kept merge cell whose range starts (or continues) here */
                        const int idx = lane + u * WAVE;
                        const int lo = (int) off_[u], hi = lo + tot[u];
                        if (tot[u] > 0 && hi > q0 && lo < q0 + 512) heads[lo > q0 ? lo - q0 : 0] = (uint32_t) idx + 1u;
                    }
                    wave_lds_fence();
                    uint32_t own[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        own[j] = 0u;
                        if (j < ns) { own[j] = heads[j * WAVE + lane]; heads[j * WAVE + lane] = 0u; } /* left clean for the next use */
                    }
                    uint32_t carry = 0u; /* the latest mark of the slots before */
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (j < ns) { /* inclusive prefix maximum over the lanes (marks grow with the position: max = latest) */
                            uint32_t v = own[j], t;
                            t = dpp_mov<0x111>(v); if ((lane & 15) >= 1) v = t > v ? t : v;
                            t = dpp_mov<0x112>(v); if ((lane & 15) >= 2) v = t > v ? t : v;
                            t = dpp_mov<0x114>(v); if ((lane & 15) >= 4) v = t > v ? t : v;
                            t = dpp_mov<0x118>(v); if ((lane & 15) >= 8) v = t > v ? t : v;
                            t = dpp_mov<0x142, 0xa>(v); if ((lane & 31) >= 16) v = t > v ? t : v;
                            t = dpp_mov<0x143, 0xc>(v); if (lane >= 32) v = t > v ? t : v;
                            v = v > carry ? v : carry;
                            own[j] = v;
                            carry = (uint32_t) __builtin_amdgcn_readlane((int) v, WAVE - 1);
                        }
                    }
                    uint32_t w0[8], w1[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        key[j] = 0xFFFFFFFFu;
                        if (j < ns) {
                            const bool act = j * WAVE + lane < left && own[j] > 0u;
                            const uint2 r = act ? *reinterpret_cast<const uint2 *>(minfo + 2 * (own[j] - 1u)) : make_uint2(0u, 0u);
                            w0[j] = r.x; w1[j] = r.y;
                            if (act) key[j] = 0u;
                        }
                    }
                    uint32_t c1_[8], c2_[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (j < ns) {
                            const uint32_t nbq = (w0[j] >> 14) & 0xFFu, off = w1[j] & 0x3FFFu, sa = (w1[j] >> 14) & 0x7Fu, sb = (w1[j] >> 21) & 0x7Fu;
                            const uint32_t t = (uint32_t) (q0 + j * WAVE + lane) - off;
                            /* t = x * nb + y, nb <= 128: exact through a float reciprocal (t < 2^14) */
                            uint32_t x = (uint32_t) ((float) t * __builtin_amdgcn_rcpf((float) (nbq ? nbq : 1u)));
                            if (x * nbq > t) x--;
                            if ((x + 1u) * nbq <= t) x++;
                            const uint32_t y = t - x * nbq;
                            c1_[j] = listA[(sa + x) & 127u];
                            c2_[j] = listB[(sb + y) & 127u];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (j < ns) {
                            const uint32_t e = key[j] == 0u ? pair_index(c1_[j], c2_[j], C2, inv, a_cp, b_cp) : 0u;
                            aux[j] = c1_[j] | (c2_[j] << 8) | ((w0[j] & 0x3FFFu) << 16);
                            const uint32_t bin_ = bin_k[e];
                            if (key[j] == 0u) key[j] = (bin_ << 14) | e;
                        }
                    }
                    return ns;
                };
                /* a selected candidate: its slot of the selection, and -- the first time its next merge cell is seen -- that merge
                 * cell as a kept merge cell of the next column.  Called in wave-uniform control flow, `take` per lane. */
                int cm = 0;
                auto emit = [&](bool take, int pos, uint32_t key_, uint32_t aux_) {
                    const uint32_t ii = nxA[aux_ & 0x7Fu], jj = nxB[(aux_ >> 8) & 0x7Fu];
                    const uint32_t nxt = has_next ? pair_index(ii, jj, Mb, inv, out_ap, out_bp) : 0u;
                    if (take) { skey[pos] = key_; snp[pos] = nxt | (aux_ & 0xFFFF0000u); }
                    if (has_next) {
                        bool first = false;
                        if (take) {
                            const uint32_t bit = 1u << (nxt & 31u);
                            first = (atomicOr(&bmp_m[(nxt >> 5) & 511u], bit) & bit) == 0u;
                        }
                        const uint64_t fm = __ballot(first);
                        if (first) kmn[cm + __popcll(fm & lt_mask)] = nxt | (ii << 14) | (jj << 21);
                        cm += __popcll(fm);
                    }
                };
                const int n_chunks = (L + 511) >> 9;
                int n = 0;
                if (keep_all) {
                    SEC_COUNT(8);
                    int at = 0;
                    for (int c = 0; c < n_chunks; c++) {
                        const int ns = load_chunk(c << 9);
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            if (j < ns) {
                                const bool act = key[j] != 0xFFFFFFFFu;
                                const uint64_t am = __ballot(act);
                                emit(act, at + __popcll(am & lt_mask), key[j], aux[j]);
                                at += __popcll(am);
                            }
                        }
                    }
                    n = at;
                    SEC(1);
                } else if (L <= 4 * WAVE) {
                    /* Up to four slots of candidates: selection by SORTING.  The keys bin << 14 | cell are distinct and their ascending
                     * order is the stable descending-posterior order of the reference (hmm.c:1043, :1071: smaller bin = larger
                     * posterior, ties in list order = cell index): the kept cells are the first n of the sorted candidates.  One
                     * bitonic sort in registers over as many slots as the column needs replaces histogram, cutoff search,
                     * selection pass and tie ranking (measured: 29 000 cycles per such column against 10 000 for a column that
                     * keeps all its candidates).  What rides along with a candidate (its parent cells, the merge cell it comes
                     * from) is re-derived from the cell index for the kept ones. */
                    SEC_COUNT(9);
                    const int ns = load_chunk(0);
                    int g = L;
                    if (!thr_all) {
                        g = 0;
#pragma unroll
                        for (int j = 0; j < 8; j++)
                            if (j < ns) g += __popcll(__ballot(key[j] != 0xFFFFFFFFu && (int) (key[j] >> 14) <= p.thr_bin));
                    }
                    n = kept_count(L, g, p.min_p, p.max_p);
                    if (ns <= 2) { uint32_t kk[2] = {key[0], key[1]}; wave_bitonic_sort_n<2>(kk, lane); key[0] = kk[0]; key[1] = kk[1]; }
                    else { uint32_t kk[4] = {key[0], key[1], key[2], key[3]}; wave_bitonic_sort_n<4>(kk, lane); key[0] = kk[0]; key[1] = kk[1]; key[2] = kk[2]; key[3] = kk[3]; }
                    const uint32_t Pb = cd1 >> 16;
                    const bool in_ap = (cflags & MRP_XF_IN_A_PAIRED) != 0, in_bp = (cflags & MRP_XF_IN_B_PAIRED) != 0;
                    const uint32_t *pvA = tA + 512, *pvB = tB + 512;
                    const float rc2 = __builtin_amdgcn_rcpf((float) (C2 ? C2 : 1u)), rc22 = __builtin_amdgcn_rcpf((float) (C2 ? 2u * C2 : 1u));
#pragma unroll
                    for (int j = 0; j < 2; j++) { /* n <= S <= 128: the kept cells are in the first two registers */
                        if (j * WAVE < n) {
                            const bool take = j * WAVE + lane < n;
                            const uint32_t e = take ? key[j] & 0x3FFFu : 0u;
                            uint32_t c1, c2; /* cross_cell(e), the divisions through float reciprocals (exact: e < 2^14, one correction step) */
                            if (!inv) {
                                uint32_t q = (uint32_t) ((float) e * rc2);
                                if (q * C2 > e) q--;
                                if ((q + 1u) * C2 <= e) q++;
                                c1 = q; c2 = e - q * C2;
                            } else if (!a_cp) { c1 = 0u; c2 = e; }
                            else {
                                uint32_t r = (uint32_t) ((float) e * rc22);
                                if (r * 2u * C2 > e) r--;
                                if ((r + 1u) * 2u * C2 <= e) r++;
                                const uint32_t t = e - r * 2u * C2, hh = t >> 1;
                                if (t & 1u) { c1 = 2u * r + 1u; c2 = b_cp ? (hh ^ 1u) : hh; } else { c1 = 2u * r; c2 = hh; }
                            }
                            c1 &= 127u; c2 &= 127u;
                            const uint32_t prv = k > 0 ? pair_index(pvA[c1], pvB[c2], Pb, inv, in_ap, in_bp) : 0u;
                            emit(take, j * WAVE + lane, key[j], c1 | (c2 << 8) | (prv << 16));
                        }
                    }
                    SEC(4);
                } else {
                    /* pass 1: histogram of the posterior bins */
                    SEC_COUNT(n_chunks > 1 ? 11 : 10);
                    int ns = 0;
                    for (int c = 0; c < n_chunks; c++) {
                        ns = load_chunk(c << 9);
#pragma unroll
                        for (int j = 0; j < 8; j++)
                            if (j < ns && key[j] != 0xFFFFFFFFu) {
                                const int bin_ = (int) (key[j] >> 14);
                                atomicAdd(&hk[(bin_ & 15) * WAVE + (bin_ >> 4)], 1u);
                            }
                    }
                    wave_lds_fence();
                    SEC(2);
                    /* cutoff bin and quota: lane l owns the 16 consecutive bins [16 l, 16 l + 16); the histogram is stored
                     * lane-major, so these reads are conflict-free and the search has a fixed, short cost */
                    int v[16];
                    int tot_l = 0, pass = 0;
                    const int thr_rel = p.thr_bin - lane * 16; /* bins q <= thr_rel of this lane pass the threshold */
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        v[q] = (int) hk[q * WAVE + lane];
                        tot_l += v[q];
                        if (q <= thr_rel) pass += v[q];
                    }
                    const int incl = wave_incl_scan(tot_l, lane);
                    const int g = thr_all ? L : __builtin_amdgcn_readlane(wave_incl_scan(pass, lane), WAVE - 1);
                    n = kept_count(L, g, p.min_p, p.max_p);
                    const int ex = incl - tot_l;
                    int myq = -1, myQ = 0, myV = 0;
                    const bool owner_lane = n > 0 && ex < n && n <= incl;
                    if (owner_lane) {
                        int cum = ex;
#pragma unroll
                        for (int q = 0; q < 16; q++) {
                            if (myq < 0 && cum + v[q] >= n) { myq = q; myQ = n - cum; myV = v[q]; }
                            cum += v[q];
                        }
                    }
                    const int myB = lane * 16 + myq;
                    const uint64_t om = __ballot(owner_lane);
                    const int srcu = __builtin_amdgcn_readfirstlane(om ? __ffsll((unsigned long long) om) - 1 : 0);
                    const int B = om ? __builtin_amdgcn_readlane(myB, srcu) : -1;
                    const int quota = om ? __builtin_amdgcn_readlane(myQ, srcu) : 0;
                    const int in_B = om ? __builtin_amdgcn_readlane(myV, srcu) : 0;
                    const int nG = n - quota;
                    const bool whole_bin = in_B == quota; /* the cutoff bin is kept entirely: no ranking needed */
                    SEC(3);
                    /* pass 2: the cells above the cutoff bin; those in it are kept directly or marked by cell index */
                    int gc = 0, ec = 0;
                    for (int c = 0; c < n_chunks; c++) {
                        if (n_chunks > 1) ns = load_chunk(c << 9); /* a single chunk is still in the registers */
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            if (j >= ns) continue;
                            const int bin_ = key[j] != 0xFFFFFFFFu ? (int) (key[j] >> 14) : nb;
                            const bool is_g = bin_ < B, is_e = bin_ == B;
                            const uint64_t mg = __ballot(is_g), me = __ballot(is_e);
                            const bool take = is_g || (is_e && whole_bin);
                            emit(take, is_g ? gc + __popcll(mg & lt_mask) : nG + ec + __popcll(me & lt_mask), key[j], aux[j]);
                            if (is_e && !whole_bin) {
                                const uint32_t e = key[j] & 0x3FFFu;
                                atomicOr(&bmp_c[e >> 5], 1u << (e & 31u));
                            }
                            gc += __popcll(mg);
                            ec += __popcll(me);
                        }
                    }
                    SEC(4);
                    if (!whole_bin && quota > 0) {
                        /* the first `quota` cells of the cutoff bin in list order (= by cell index): a cell's rank is the number
                         * of marks below it -- marks before its bitmap word (prefix counts, lane l owns words 8 l .. 8 l + 7) plus
                         * those below it in the word */
                        wave_lds_fence();
                        {
                            uint32_t w[8];
                            int cnt_l = 0;
#pragma unroll
                            for (int q = 0; q < 8; q++) { w[q] = bmp_c[lane * 8 + q]; cnt_l += __popc(w[q]); }
                            int run = wave_incl_scan(cnt_l, lane) - cnt_l;
#pragma unroll
                            for (int q = 0; q < 8; q++) { pref[lane * 8 + q] = (uint32_t) run; run += __popc(w[q]); }
                        }
                        wave_lds_fence();
                        for (int c = 0; c < n_chunks; c++) {
                            if (n_chunks > 1) ns = load_chunk(c << 9);
#pragma unroll
                            for (int j = 0; j < 8; j++) {
                                if (j >= ns) continue;
                                const bool is_e = key[j] != 0xFFFFFFFFu && (int) (key[j] >> 14) == B;
                                const uint32_t e = key[j] & 0x3FFFu, wd = is_e ? e >> 5 : 0u;
                                const int rank = (int) pref[wd] + __popc(bmp_c[wd] & ((1u << (e & 31u)) - 1u));
                                emit(is_e && rank < quota, nG + rank, key[j], aux[j]);
                            }
                        }
                        wave_lds_fence();
                        for (int c = 0; c < n_chunks; c++) { /* the marks go */
                            if (n_chunks > 1) ns = load_chunk(c << 9);
#pragma unroll
                            for (int j = 0; j < 8; j++)
                                if (j < ns && key[j] != 0xFFFFFFFFu && (int) (key[j] >> 14) == B) bmp_c[(key[j] & 0x3FFFu) >> 5] = 0u;
                        }
                    }
                }
                wave_lds_fence();
                SEC(5);
                if (lane == 0) { sh[32 + b] = (uint32_t) n; sh[40 + (b ^ 1)] = (uint32_t) cm; }
                /* the marks of the next merge cells go */
                if (has_next) {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int idx = lane + u * WAVE;
                        if (idx < cm) bmp_m[((kmn[idx] & 0x3FFFu) >> 5) & 511u] = 0u;
                    }
                }
                SEC(6);
                ROLE_BARRIER();
            }
            } /* PAIRS or not */
            ROLE_CLK_DONE(0);
            SEC_DONE();
            lds_barrier();
            if (PAIRS) lds_barrier(); /* (the list stages of the chain on pairs run three columns deep) */
        } else if (wave == 1) {
            int64_t mcell_prev = 0; /* first merge cell of the merge column after column k - 1 */
            SweepCol scur = k_load(d.scols + h.col0);
            lds_barrier();
            ROLE_CLK_INIT();
            if constexpr (PAIRS) {
                for (int k = 0; k < K; k++) {
                    if (k > 1) stage1_finish(k - 2);
                    if (k > 0) stage1_ask(k - 1, mcell_prev);
                    mcell_prev = scur.mcell_off;
                    if (k + 1 < K) scur = k_load(d.scols + h.col0 + k + 1);
                    ROLE_BARRIER();
                }
                ROLE_CLK_DONE(1);
                if (K > 1) stage1_finish(K - 2);
                stage1_ask(K - 1, mcell_prev);
                lds_barrier();
                stage1_finish(K - 1);
                lds_barrier();
            } else {
                for (int k = 0; k < K; k++) {
                    if (k > 0) lists_stage1(k - 1, mcell_prev);
                    mcell_prev = scur.mcell_off;
                    if (k + 1 < K) scur = k_load(d.scols + h.col0 + k + 1);
                    ROLE_BARRIER();
                }
                ROLE_CLK_DONE(1);
                lists_stage1(K - 1, mcell_prev);
                lds_barrier();
            }
        } else if (wave == 2) {
            lds_barrier();
            ROLE_CLK_INIT();
            if constexpr (PAIRS) { /* a column later than the general chain: stage 1 takes two steps */
                for (int k = 0; k < K; k++) {
                    if (k > 2) lists_stage2(k - 3);
                    ROLE_BARRIER();
                }
                ROLE_CLK_DONE(2);
                if (K > 2) lists_stage2(K - 3);
                lds_barrier();
                if (K > 1) lists_stage2(K - 2);
                lds_barrier();
                lists_stage2(K - 1);
            } else {
                for (int k = 0; k < K; k++) {
                    if (k > 1) lists_stage2(k - 2);
                    ROLE_BARRIER();
                }
                ROLE_CLK_DONE(2);
                if (K > 1) lists_stage2(K - 2);
                lds_barrier();
                lists_stage2(K - 1);
            }
        } else if (wave == 3) {
            /* wave 3: the parents' transitions of the column after next.  Three columns are in the pipe: the tables of column
             * t are built from the registers while the transitions of column t + 1 and the descriptor of column t + 2 are in
             * flight.  The descriptors come by VECTOR loads (lane l = dword l of the CrossCol, lanes 16.. = the SweepCol) and
             * are taken apart with v_readlane a step later: a scalar load shares lgkmcnt with the LDS traffic of the table
             * build, and a wave that first has to wait for its descriptor before it can ask for the transitions it points to
             * pays two memory latencies per column -- with the chain on complement pairs this wave had become the slowest role. */
            uint32_t r_na[2] = {0u, 0u}, r_nb[2] = {0u, 0u};
            int32_t t_f[W == 4 ? CPT : 1], t_b[W == 4 ? CPT : 1]; /* T = 256: f and b of the column whose tables are built next */
            int t_n = 0;
            CrossCol tcc = {};
            int tcol = 0;
            auto desc_load = [&](int col) -> uint32_t {
                uint32_t v = 0u;
                if (col < K) {
                    if (lane < 16) v = reinterpret_cast<const uint32_t *>(d.ccols + h.col0 + col)[lane];
                    else if (W == 4 && lane < 24) v = reinterpret_cast<const uint32_t *>(d.scols + h.col0 + col)[lane - 16];
                }
                return v;
            };
            auto fld = [&](uint32_t v, int l) -> uint32_t { return (uint32_t) __builtin_amdgcn_readlane((int) v, l); };
            /* the transitions (and, T = 256, f and b) of the column the descriptor vector dv describes: requests only */
            auto tab_load = [&](uint32_t dv) {
                CrossCol c = {};
                c.a_part = reinterpret_cast<const uint64_t *>(((uint64_t) fld(dv, 1) << 32) | fld(dv, 0));
                c.b_part = reinterpret_cast<const uint64_t *>(((uint64_t) fld(dv, 3) << 32) | fld(dv, 2));
                c.a_np = reinterpret_cast<const uint32_t *>(((uint64_t) fld(dv, 5) << 32) | fld(dv, 4));
                c.b_np = reinterpret_cast<const uint32_t *>(((uint64_t) fld(dv, 7) << 32) | fld(dv, 6));
                const uint32_t w10 = fld(dv, 10), w11 = fld(dv, 11), w12 = fld(dv, 12), w13 = fld(dv, 13), w14 = fld(dv, 14);
                c.C1 = (uint16_t) w10; c.C2 = (uint16_t) (w10 >> 16); c.Ma = (uint16_t) w11; c.Mb = (uint16_t) (w11 >> 16);
                c.Pa = (uint16_t) w12; c.Pb = (uint16_t) (w12 >> 16);
                c.d1 = (uint8_t) w13; c.d2 = (uint8_t) (w13 >> 8); c.out_a = (uint8_t) (w13 >> 16); c.out_b = (uint8_t) (w13 >> 24);
                c.in_a = (uint8_t) w14; c.in_b = (uint8_t) (w14 >> 8); c.flags = (uint8_t) (w14 >> 16);
                tcc = c;
                if (tcol < K) {
                    if (W == 4) {
                        const int64_t cell_off = (int64_t) (((uint64_t) fld(dv, 17) << 32) | fld(dv, 16));
                        t_n = (int) fld(dv, 20);
#pragma unroll
                        for (int j = 0; j < (W == 4 ? CPT : 1); j++) {
                            const int cell = lane + j * WAVE;
                            t_f[j] = cell < t_n ? d.cell_f32[cell_off + cell] : MRP_NEG_I32;
                            t_b[j] = cell < t_n ? d.cell_b32[cell_off + cell] : MRP_NEG_I32;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const uint32_t cidx = (uint32_t) (lane + u * WAVE);
                        r_na[u] = (tcc.a_np && cidx < tcc.C1) ? tcc.a_np[cidx] : 0u;
                        r_nb[u] = (tcc.b_np && cidx < tcc.C2) ? tcc.b_np[cidx] : 0u;
                    }
                }
            };
            /* inverted transition lists of both sides (cells grouped by the merge cell they come from: count, first entry, list),
             * the two sides side by side between the same three LDS fences */
            auto tab_build_sides = [&](uint32_t *tA5, uint32_t CA, uint32_t PA, uint32_t in_a, uint32_t out_a, uint32_t CB, uint32_t PB, uint32_t in_b, uint32_t out_b) {
                uint32_t *t5[2] = {tA5, tA5 + PRUNE_TAB * 128};
                const uint32_t C_[2] = {CA, CB}, in_[2] = {in_a, in_b}, out_[2] = {out_a, out_b};
                const uint32_t G_[2] = {PA < 1u ? 1u : (PA > 128u ? 128u : PA), PB < 1u ? 1u : (PB > 128u ? 128u : PB)};
#pragma unroll
                for (int sd = 0; sd < 2; sd++) { t5[sd][lane] = 0u; t5[sd][lane + WAVE] = 0u; }
                wave_lds_fence();
                uint32_t rank[2][2] = {{0u, 0u}, {0u, 0u}}, grp_[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
                for (int sd = 0; sd < 2; sd++) {
                    uint32_t *cnt = t5[sd], *nx = t5[sd] + 384, *pv = t5[sd] + 512;
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const uint32_t c = (uint32_t) (lane + u * WAVE);
                        const uint32_t rn = sd == 0 ? r_na[u] : r_nb[u];
                        if (c < C_[sd]) {
                            uint32_t pvi = in_[sd] == MRP_CONN_REAL ? (rn >> 16) : (in_[sd] == MRP_CONN_IDENT ? c : 0u);
                            const uint32_t nxi = out_[sd] == MRP_CONN_REAL ? (rn & 0xFFFFu) : (out_[sd] == MRP_CONN_IDENT ? c : 0u);
                            if (pvi >= G_[sd]) { errbits |= MRP_ENGINE_ERR_RANGE; pvi = 0u; }
                            pv[c] = pvi; nx[c] = nxi;
                            grp_[sd][u] = pvi;
                            rank[sd][u] = atomicAdd(&cnt[pvi], 1u);
                        }
                    }
                }
                wave_lds_fence();
                /* exclusive scan of the group sizes (two per lane and side: groups lane and lane + 64) */
                int c0[2], c1[2], i0[2], i1[2];
#pragma unroll
                for (int sd = 0; sd < 2; sd++) { c0[sd] = (int) t5[sd][lane]; c1[sd] = (int) t5[sd][lane + WAVE]; }
#pragma unroll
                for (int sd = 0; sd < 2; sd++) { i0[sd] = wave_incl_scan_bc(c0[sd]); i1[sd] = wave_incl_scan_bc(c1[sd]); }
#pragma unroll
                for (int sd = 0; sd < 2; sd++) {
                    uint32_t *start = t5[sd] + 128;
                    const int t0 = __builtin_amdgcn_readlane(i0[sd], WAVE - 1);
                    /* (the chain on pairs reads a group's first entry and size as one word) */
                    start[lane] = (uint32_t) (i0[sd] - c0[sd]) | (PAIRS ? (uint32_t) c0[sd] << 8 : 0u);
                    start[lane + WAVE] = (uint32_t) (t0 + i1[sd] - c1[sd]) | (PAIRS ? (uint32_t) c1[sd] << 8 : 0u);
                }
                wave_lds_fence();
#pragma unroll
                for (int sd = 0; sd < 2; sd++) {
                    uint32_t *start = t5[sd] + 128, *list = t5[sd] + 256;
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const uint32_t c = (uint32_t) (lane + u * WAVE);
                        if (c < C_[sd]) list[(start[grp_[sd][u]] & 0xFFu) + rank[sd][u]] = c;
                    }
                }
            };
            auto tab_build = [&]() { /* tables of column tcol into buffer tcol & 1, from the registers loaded last time */
                if (tcol < K) {
                    uint32_t *tb = tab + (tcol & 1) * 2 * PRUNE_TAB * 128;
                    if (lane == 0) { /* the chain's view of the column (read after the barrier that ends this step) */
                        sh[48 + 4 * (tcol & 1)] = (uint32_t) tcc.C2 | ((uint32_t) tcc.Mb << 16);
                        sh[49 + 4 * (tcol & 1)] = (uint32_t) tcc.flags | ((tcc.a_part && tcc.d1 > 0) ? 0x100u : 0u) | ((tcc.b_part && tcc.d2 > 0) ? 0x200u : 0u) |
                                                  ((uint32_t) tcc.Pb << 16);
                        if (PAIRS) { /* what the chain on pairs derives from these flags, as bits (see its unit() / parity() rule) */
                            const bool a_cp = tcc.a_part && tcc.d1 > 0, b_cp = tcc.b_part && tcc.d2 > 0;
                            const bool o_a = (tcc.flags & MRP_XF_OUT_A_PAIRED) != 0, o_b = (tcc.flags & MRP_XF_OUT_B_PAIRED) != 0;
                            const bool i_a = (tcc.flags & MRP_XF_IN_A_PAIRED) != 0, i_b = (tcc.flags & MRP_XF_IN_B_PAIRED) != 0;
                            sh[50 + 4 * (tcol & 1)] = ((a_cp && b_cp) ? 1u : 0u) | ((!a_cp && b_cp) ? 2u : 0u) | (a_cp ? 4u : 0u) | ((o_a && o_b) ? 8u : 0u) |
                                                      ((!o_a && o_b) ? 16u : 0u) | (o_a ? 32u : 0u) | ((o_a || o_b) ? 64u : 0u) | ((i_a || i_b) ? 128u : 0u) |
                                                      (i_a ? 256u : 0u) | ((!i_a && i_b) ? 512u : 0u) | ((a_cp || b_cp) ? 1024u : 0u) |
                                                      ((!(i_a || i_b) && (a_cp || b_cp)) ? 2048u : 0u);
                        }
                    }
                    if (W == 4) { /* the column's posterior bins */
                        uint16_t *dst = bins + (tcol & 1) * cap_c;
                        if (t_n > CPT * WAVE) { errbits |= MRP_ENGINE_ERR_RANGE; t_n = CPT * WAVE; }
#pragma unroll
                        for (int j = 0; j < (W == 4 ? CPT : 1); j++) {
                            const int cell = lane + j * WAVE;
                            if (PAIRS && !units) { if (cell < t_n && (cell & 1) == 0) dst[cell >> 1] = (uint16_t) posterior_bin(t_f[j], t_b[j], total, nb, &errbits); }
                            else if (cell < t_n) dst[cell] = (uint16_t) posterior_bin(t_f[j], t_b[j], total, nb, &errbits);
                        }
                    }
                    uint32_t C1 = tcc.C1, C2 = tcc.C2;
                    if (C1 > 128u || C2 > 128u) { errbits |= MRP_ENGINE_ERR_RANGE; C1 = C1 > 128u ? 128u : C1; C2 = C2 > 128u ? 128u : C2; }
                    tab_build_sides(tb, C1, tcc.Pa, tcc.in_a, tcc.out_a, C2, tcc.Pb, tcc.in_b, tcc.out_b);
                }
            };

            /* the parents' transitions: tables of column 0, requests for column 1, descriptor of column 2 */
            uint32_t dv_next;
            tcol = 0; tab_load(desc_load(0)); tab_build();
            tcol = 1; tab_load(desc_load(1));
            dv_next = desc_load(2);
            lds_barrier();
            ROLE_CLK_INIT();
            for (int k = 0; k < K; k++) {
                /* tables of column k + 1 (requested while column k - 1 was worked on), then the requests for k + 2 (its
                 * descriptor was requested a step ago) and the descriptor of k + 3 */
                tab_build();
                tcol++;
                tab_load(dv_next);
                dv_next = desc_load(k + 3);
                uint32_t *hn = hist + ((k + 1) & 1) * nb_r;
                if (!PAIRS || sh[56 + ((k + 1) & 1)] != 0u) { /* (the chain on pairs says when it has used a histogram: one column in a hundred) */
                    for (int i = lane; i < nb_r; i += WAVE) hn[i] = 0u;
                    if (PAIRS && lane == 0) sh[56 + ((k + 1) & 1)] = 0u;
                }
                ROLE_BARRIER();
            }
            ROLE_CLK_DONE(3);
            lds_barrier();
            if (PAIRS) lds_barrier();
        } else {
            /* bins groups (waves 4..): group g handles the columns g, g + 2, ...  A step of its loop stores the bins of the
             * column whose f and b sit in the registers and requests the column after next into the same registers; the
             * group is idle during the other group's step.  Loads are issued for every register slot whatever the column's
             * size (beyond the column -- and beyond the last column -- the buffer descriptor's range check returns 0 without
             * touching memory): a load under a condition would make every slot a loop-carried merge of old and new value,
             * which costs a second register set. */
            int32_t r_f[CPT * VEC], r_b[CPT * VEC];
            const int bw = wave - 4, grp = NGRP == 2 ? (bw & 1) : 0, gidx = NGRP == 2 ? (bw >> 1) : bw;
            const int base_c = gidx * WAVE + lane, voff = base_c * 4 * VEC;
            int n_have = 0; /* cells of the column in the registers */
            auto bins_load = [&](int col) {
                const bool valid = col < K;
                const SweepCol c = k_load(d.scols + h.col0 + (valid ? col : 0));
                n_have = valid ? c.n_cells : 0;
                /* (VEC = 4: the last load of a column reads up to three cells of what follows it -- the hmm's cells are padded
                 * to a multiple of four, the arrays end with slack -- and bins_store leaves them out) */
                const int bytes_ = __builtin_amdgcn_readfirstlane(((n_have + VEC - 1) & ~(VEC - 1)) * 4);
                const auto rf_ = prune_rsrc(d.cell_f32 + c.cell_off, bytes_);
                const auto rb_ = prune_rsrc(d.cell_b32 + c.cell_off, bytes_);
#pragma unroll
                for (int j = 0; j < CPT; j++) { /* one lane offset for all loads; the step from load to load rides in the scalar offset */
                    if (VEC == 1) {
                        r_f[j] = (int32_t) __builtin_amdgcn_raw_buffer_load_b32(rf_, voff, j * LG * 4, 0);
                        r_b[j] = (int32_t) __builtin_amdgcn_raw_buffer_load_b32(rb_, voff, j * LG * 4, 0);
                    } else {
                        const auto vf = __builtin_amdgcn_raw_buffer_load_b128(rf_, voff, j * LG * 16, 0);
                        const auto vb = __builtin_amdgcn_raw_buffer_load_b128(rb_, voff, j * LG * 16, 0);
#pragma unroll
                        for (int q = 0; q < VEC; q++) { r_f[j * VEC + q] = (int32_t) vf[q]; r_b[j * VEC + q] = (int32_t) vb[q]; }
                    }
                }
            };
            auto bins_store = [&](int col) { /* the bins of column col into buffer col & 1 */
                uint16_t *dst = bins + (col & 1) * cap_c;
                const int nj = (n_have + LG * VEC - 1) / (LG * VEC);
#pragma unroll
                for (int j = 0; j < CPT; j++) {
                    if (j < nj) { /* (the lane's cell against a scalar bound, the step in the store's immediate offset: no
                                   * per-slot index registers) */
                        if (VEC == 1) {
                            if (PAIRS && !units) { /* the even cell of a unit writes the unit's bin */
                                if (base_c < n_have - j * LG && (base_c & 1) == 0) dst[(base_c + j * LG) >> 1] = (uint16_t) posterior_bin(r_f[j], r_b[j], total, nb, &errbits);
                            } else if (base_c < n_have - j * LG) dst[base_c + j * LG] = (uint16_t) posterior_bin(r_f[j], r_b[j], total, nb, &errbits);
                        } else {
                            const int left = n_have - (j * LG + base_c) * VEC; /* cells of this load inside the column */
                            if (left > 0) {
                                if (PAIRS && !units) { /* four cells = two units: the bins of cells 0 and 2 as one dword */
                                    const uint32_t b0 = (uint32_t) posterior_bin(r_f[j * VEC], r_b[j * VEC], total, nb, &errbits);
                                    const uint32_t b1 = left > 2 ? (uint32_t) posterior_bin(r_f[j * VEC + (VEC > 2 ? 2 : 0)], r_b[j * VEC + (VEC > 2 ? 2 : 0)], total, nb, &errbits) : 0u;
#ifdef MRP_PRUNE_CHECK_PAIRS /* development: the twins' f and b really are equal */
                                    if (left > 1 && (r_f[j * VEC] != r_f[j * VEC + 1] || r_b[j * VEC] != r_b[j * VEC + 1])) errbits |= MRP_ENGINE_ERR_STRUCTURE;
                                    if (left > 3 && (r_f[j * VEC + 2] != r_f[j * VEC + 3] || r_b[j * VEC + 2] != r_b[j * VEC + 3])) errbits |= MRP_ENGINE_ERR_STRUCTURE;
#endif
                                    *reinterpret_cast<uint32_t *>(dst + (j * LG + base_c) * (VEC / 2)) = b0 | (b1 << 16);
                                } else {
                                    uint32_t bq[VEC];
#pragma unroll
                                    for (int q = 0; q < VEC; q++) bq[q] = q < left ? (uint32_t) posterior_bin(r_f[j * VEC + q], r_b[j * VEC + q], total, nb, &errbits) : 0u;
                                    *reinterpret_cast<uint2 *>(dst + (j * LG + base_c) * VEC) = make_uint2(bq[0] | (bq[VEC > 1 ? 1 : 0] << 16), bq[VEC > 2 ? 2 : 0] | (bq[VEC > 3 ? 3 : 0] << 16));
                                }
                            }
                        }
                    }
                }
            };
            ROLE_CLK_INIT();
            if (NGRP == 2) {
                /* barrier schedule: one after the prologue (step -1), one per column (steps 0 .. K - 1), one before the last merge
                 * list.  Group 0 acts at steps -1, 1, 3, ... (columns 0, 2, 4, ...), group 1 at steps 0, 2, ... */
                bins_load(grp);
                if (grp == 1) lds_barrier(); /* step -1 */
                for (int st = grp - 1; st < K; st += 2) {
                    bins_store(st + 1);
                    __builtin_amdgcn_sched_barrier(0); /* the new column's loads reuse the registers of the one just stored */
                    bins_load(st + 3);
                    ROLE_BARRIER();                 /* end of step st */
                    if (st + 1 < K) ROLE_BARRIER(); /* step st + 1: the other group's */
                }
            } else {
                /* one group: at step st the bins of column st + 1 (requested during step st - 1) are stored and column st + 2
                 * is requested: a column's f and b have one column time to arrive */
                bins_load(0);
                for (int st = -1; st < K; st++) {
                    bins_store(st + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    bins_load(st + 2);
                    ROLE_BARRIER(); /* end of step st */
                }
            }
            if (gidx == 0) ROLE_CLK_DONE(4 + grp);
            lds_barrier();
            if (PAIRS) lds_barrier();
        }
        __syncthreads(); /* also makes the lists above visible in global memory */

        /* (stRPHmm_pruneBackwards runs as a kernel of its own, mrp_prune_back_kernel: one wave per hmm instead of one wave of eight for a
         * quarter of this workgroup's life) */
        if (errbits) { atomicOr(sc.err, errbits); atomicOr(sc.err_hmm + hi_, errbits); }
        __syncthreads();
    }
}

/*
 * stRPHmm_pruneBackwards (hmm.c:1111-1158) of a level, one WAVE per hmm.  It used to be the tail of mrp_prune_kernel, run by the chain
 * wave while the workgroup's other seven waves -- and their registers, half a CU's -- waited: 1.3-1.9 M of a top-level workgroup's 7 M
 * cycles (`-DPRUNE_EXP_CLOCK`), a quarter of the slot-time of the kernel that holds most of it.  Here it holds 64 lanes and a few hundred
 * bytes of LDS per hmm (the kept flag per merge cell).  The forward pass's lists (sc.kept, kept_np, keptm, their counts) are complete when
 * this kernel starts: same stream, behind mrp_prune_kernel.
 */
template <bool PAIRS>
__global__ void __launch_bounds__(256) mrp_prune_back_kernel(const PruneHmm *__restrict__ hmms, int64_t n_hmms, PruneParams p, PruneScratch sc) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x / WAVE));
    const int S = p.S;
    const int n_flagw = ((p.max_merge + 127) >> 7) << 2; /* words, a multiple of four */
    uint32_t *flagw = lds + wave * n_flagw;              /* [max_merge bits] kept flag per merge cell, this wave's */
    auto flag_get = [&](uint32_t i) -> bool { return (flagw[i >> 5] >> (i & 31u)) & 1u; };
    auto flag_set = [&](uint32_t i) { atomicOr(&flagw[i >> 5], 1u << (i & 31u)); };
    auto flag_clr = [&](uint32_t i) { atomicAnd(&flagw[i >> 5], ~(1u << (i & 31u))); };
    for (int i = lane; i < n_flagw; i += WAVE) flagw[i] = 0u;
    wave_lds_fence();
    for (int64_t hi_ = (int64_t) blockIdx.x * 4 + wave; hi_ < n_hmms; hi_ += (int64_t) gridDim.x * 4) {
        const PruneHmm h = k_load(hmms + hi_);
        const int K = h.n_cols;
        /* ---- stRPHmm_pruneBackwards hmm.c:1111-1158: lists of at most S entries, one wave; the lists of
         * column k - 1 are requested before column k is worked on ---- */
        if constexpr (PAIRS) {
            /* The lists in UNITS: entry i = cells 2 i, 2 i + 1 of the kept list (the list stages wrote a unit's cells next to each
             * other; a column or merge column of one cell has a list of one -- an odd count), one entry per lane, the flags one
             * per merge unit.  The merge cells the surviving cells come from are all in the forward pass's kept merge list (it
             * keeps every merge cell a kept cell leads to, checked), so the flags set from the cells are the survivors of that list. */
            struct ListsU { int nk, nm; uint32_t cc; uint2 cn; uint32_t mm; };
            auto fetch = [&](int k) {
                ListsU L;
                L.nk = 0; L.nm = 0; L.cc = 0u; L.cn = make_uint2(0u, 0u); L.mm = 0u;
                if (k >= 0) {
                    const int64_t lc = h.col0 + k;
                    L.nk = sc.n_kept[lc];
                    L.nm = sc.n_keptm[lc];
                    if (2 * lane < S) { /* (the counts are not known yet when the lists are requested: every slot below S is read) */
                        L.cc = *reinterpret_cast<const uint32_t *>(sc.kept + lc * S + 2 * lane);
                        L.cn = *reinterpret_cast<const uint2 *>(sc.kept_np + lc * S + 2 * lane);
                        L.mm = *reinterpret_cast<const uint32_t *>(sc.keptm + lc * S + 2 * lane);
                    }
                }
                return L;
            };
            uint32_t pm = 0u; /* merge unit of the merge column after column k this lane has flagged */
            bool pmk = false;
            (void) fetch;
            /* The lists of four columns are in flight at a time, in a ring of registers loaded by inline asm and waited for by count (as the
             * recursion kernel's ring, mrp_kernels.hip): through the compiler's own waits -- the lists are loop-carried registers, so it
             * waits with vmcnt(0) at the loop head -- every column paid the whole trip to HBM / L2 of the lists asked for a column earlier
             * (1 450 cycles per column for some 500 of LDS flag operations and ballots).  Memory operations retire in issue order and
             * stores share the counter: a step issues exactly FIVE ring loads (unconditionally: beyond column 0 they read column 0 and
             * are ignored) plus stores that can only make a wait stricter; when a step starts, the two entries it needs are followed
             * by the loads of two younger entries: vmcnt(10). */
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            int32_t bnk0 = 0, bnk1 = 0, bnk2 = 0, bnk3 = 0, bnm0 = 0, bnm1 = 0, bnm2 = 0, bnm3 = 0;
            uint32_t bcc0 = 0u, bcc1 = 0u, bcc2 = 0u, bcc3 = 0u, bmm0 = 0u, bmm1 = 0u, bmm2 = 0u, bmm3 = 0u;
            u32x2 bcn0 = {0u, 0u}, bcn1 = {0u, 0u}, bcn2 = {0u, 0u}, bcn3 = {0u, 0u};
            const int lane2 = 2 * lane < S ? 2 * lane : 0; /* (lanes beyond the lists read entry 0 and never use it: lane < nku <= S / 2) */
#define BK_LOAD(i, k_)                                                                                                                  \
            {                                                                                                                           \
                const int kk_ = (k_) < 0 ? 0 : (k_);                                                                                    \
                const int64_t lc_ = h.col0 + kk_;                                                                                       \
                asm volatile("global_load_dword %0, %5, off\n\tglobal_load_dword %1, %6, off\n\tglobal_load_dword %2, %7, off\n\t"       \
                             "global_load_dwordx2 %3, %8, off\n\tglobal_load_dword %4, %9, off"                                        \
                             : "=&v"(bnk##i), "=&v"(bnm##i), "=&v"(bcc##i), "=&v"(bcn##i), "=&v"(bmm##i)                                \
                             : "v"(sc.n_kept + lc_), "v"(sc.n_keptm + lc_), "v"(sc.kept + lc_ * S + lane2), "v"(sc.kept_np + lc_ * S + lane2), \
                               "v"(sc.keptm + lc_ * S + lane2)                                                                          \
                             : "memory");                                                                                               \
            }
#ifdef MRP_SAFE_WAIT /* debugging aid: drain everything */
#define BK_WAIT(i, j) asm volatile("s_waitcnt vmcnt(0)" : "+v"(bnk##i), "+v"(bnm##i), "+v"(bcc##i), "+v"(bcn##i), "+v"(bmm##i), "+v"(bnk##j), "+v"(bnm##j), "+v"(bcc##j), "+v"(bcn##j), "+v"(bmm##j)::"memory");
#else
#define BK_WAIT(i, j) asm volatile("s_waitcnt vmcnt(10)" : "+v"(bnk##i), "+v"(bnm##i), "+v"(bcc##i), "+v"(bcn##i), "+v"(bmm##i), "+v"(bnk##j), "+v"(bnm##j), "+v"(bcc##j), "+v"(bcn##j), "+v"(bmm##j)::"memory");
#endif
            /* one column: entry i holds its lists, entry j those of the column before it; entry i is then asked for column k_ - 4 */
#define BK_STEP(i, j, k_)                                                                                                               \
            {                                                                                                                           \
                const int k = (k_);                                                                                                     \
                BK_WAIT(i, j)                                                                                                           \
                const int64_t lcol = h.col0 + k;                                                                                        \
                const int c_nk = bnk##i, c_nm = bnm##i, n_nm = k > 0 ? bnm##j : 0;                                                      \
                const uint32_t c_cc = bcc##i, c_cnx = bcn##i.x, c_cny = bcn##i.y, n_mm = bmm##j;                                        \
                const int sk = (c_nk & 1) ? 0 : 1, so = (c_nm & 1) ? 0 : 1; /* cells / merge cells after the column in pairs */          \
                const int nku = c_nk >> sk;                                                                                             \
                const bool keep = lane < nku && (k + 1 == K || flag_get((c_cnx & 0xFFFFu) >> so));                                      \
                const uint64_t m0 = __ballot(keep);                                                                                     \
                const int ns = __popcll(m0);                                                                                            \
                if (pmk) flag_clr(pm);                                                                                                  \
                pmk = false;                                                                                                            \
                if (ns != nku) {                                                                                                        \
                    if (keep) {                                                                                                         \
                        const int pos = mbcnt64(m0);                                                                                    \
                        *reinterpret_cast<uint32_t *>(sc.kept + lcol * S + 2 * pos) = c_cc;                                             \
                        *reinterpret_cast<uint2 *>(sc.kept_np + lcol * S + 2 * pos) = make_uint2(c_cnx, c_cny);                         \
                    }                                                                                                                   \
                    if (lane == 0) sc.n_kept[lcol] = ns << sk;                                                                          \
                }                                                                                                                       \
                if (k > 0) { /* merge column k - 1 keeps the merge cells some surviving cell comes from (:1141-1155) */                  \
                    const int si = (n_nm & 1) ? 0 : 1;                                                                                  \
                    if (keep) flag_set((c_cnx >> 16) >> si);                                                                            \
                    const int nmu = n_nm >> si;                                                                                         \
                    const uint32_t mu_ = (n_mm & 0xFFFFu) >> si;                                                                        \
                    const bool mk = lane < nmu && flag_get(mu_);                                                                        \
                    const uint64_t q0 = __ballot(mk);                                                                                   \
                    const int nms = __popcll(q0);                                                                                       \
                    if (nms != nmu) {                                                                                                   \
                        if (mk) *reinterpret_cast<uint32_t *>(sc.keptm + (lcol - 1) * S + 2 * mbcnt64(q0)) = n_mm;                      \
                        if (lane == 0) sc.n_keptm[lcol - 1] = nms << si;                                                                \
                    }                                                                                                                   \
                    pm = mu_; pmk = mk;                                                                                                 \
                }                                                                                                                       \
                BK_LOAD(i, k - 4)                                                                                                       \
            }
            BK_LOAD(0, K - 1) BK_LOAD(1, K - 2) BK_LOAD(2, K - 3) BK_LOAD(3, K - 4)
            for (int kq = K - 1; kq >= 0; kq -= 4) {
                BK_STEP(0, 1, kq)
                if (kq - 1 >= 0) BK_STEP(1, 2, kq - 1)
                if (kq - 2 >= 0) BK_STEP(2, 3, kq - 2)
                if (kq - 3 >= 0) BK_STEP(3, 0, kq - 3)
            }
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(bnk0), "+v"(bnk1), "+v"(bnk2), "+v"(bnk3), "+v"(bmm0), "+v"(bmm1), "+v"(bmm2), "+v"(bmm3)::"memory"); /* the ring drains before its registers are used again */
#undef BK_STEP
#undef BK_WAIT
#undef BK_LOAD
            if (pmk) flag_clr(pm);
        } else {
            uint32_t pm[2] = {0u, 0u}; /* kept merge cells of the merge column after column k: they own the flags */
            bool pmk[2] = {false, false};
            /* the lists of a column are requested two columns before they are used */
            struct Lists { int nk, nm; uint32_t cc[2], cn[2], mm[2]; };
            auto fetch = [&](int k) {
                Lists L;
                L.nk = 0; L.nm = 0;
#pragma unroll
                for (int u = 0; u < 2; u++) { L.cc[u] = 0u; L.cn[u] = 0u; L.mm[u] = 0u; }
                if (k >= 0) {
                    const int64_t lc = h.col0 + k;
                    L.nk = sc.n_kept[lc];
                    L.nm = sc.n_keptm[lc];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int i = lane + u * WAVE;
                        /* (the counts are not known yet when the lists are requested: every slot below S is read) */
                        L.cc[u] = i < S ? sc.kept[lc * S + i] : 0u;
                        L.cn[u] = i < S ? sc.kept_np[lc * S + i] : 0u;
                        L.mm[u] = i < S ? sc.keptm[lc * S + i] : 0u;
                    }
                }
                return L;
            };
            Lists cur = fetch(K - 1), nx1 = fetch(K - 2);
            for (int k = K - 1; k >= 0; k--) {
                const int64_t lcol = h.col0 + k;
                const Lists nx2 = fetch(k - 2);
                const int nk = cur.nk;
                bool keep[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int i = lane + u * WAVE;
                    keep[u] = i < nk && (k + 1 == K || flag_get(cur.cn[u] & 0xFFFFu));
                }
                const uint64_t m0 = __ballot(keep[0]), m1 = __ballot(keep[1]);
                const int ns = __popcll(m0) + __popcll(m1);
                if (pmk[0]) flag_clr(pm[0]);
                if (pmk[1]) flag_clr(pm[1]);
                if (ns != nk) {
                    if (keep[0]) {
                        const int pos = (int) lanemask_lt_count(m0, lane);
                        sc.kept[lcol * S + pos] = (uint16_t) cur.cc[0];
                        sc.kept_np[lcol * S + pos] = cur.cn[0];
                    }
                    if (keep[1]) {
                        const int pos = __popcll(m0) + (int) lanemask_lt_count(m1, lane);
                        sc.kept[lcol * S + pos] = (uint16_t) cur.cc[1];
                        sc.kept_np[lcol * S + pos] = cur.cn[1];
                    }
                    if (lane == 0) sc.n_kept[lcol] = ns;
                }
                if (k == 0) break;
                /* merge column k - 1 keeps the merge cells some surviving cell comes from (:1141-1155) */
                if (keep[0]) flag_set(cur.cn[0] >> 16);
                if (keep[1]) flag_set(cur.cn[1] >> 16);
                const int nmp = nx1.nm;
                bool mk[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int i = lane + u * WAVE;
                    mk[u] = i < nmp && flag_get(nx1.mm[u]);
                }
                const uint64_t q0 = __ballot(mk[0]), q1 = __ballot(mk[1]);
                const int nms = __popcll(q0) + __popcll(q1);
                if (nms != nmp) {
                    if (mk[0]) sc.keptm[(lcol - 1) * S + (int) lanemask_lt_count(q0, lane)] = (uint16_t) nx1.mm[0];
                    if (mk[1]) sc.keptm[(lcol - 1) * S + __popcll(q0) + (int) lanemask_lt_count(q1, lane)] = (uint16_t) nx1.mm[1];
                    if (lane == 0) sc.n_keptm[lcol - 1] = nms;
                }
                /* leave flagged exactly the surviving merge cells of column k - 1 */
                if (keep[0]) flag_clr(cur.cn[0] >> 16);
                if (keep[1]) flag_clr(cur.cn[1] >> 16);
                wave_lds_fence();
                if (mk[0]) flag_set(nx1.mm[0]);
                if (mk[1]) flag_set(nx1.mm[1]);
                pm[0] = nx1.mm[0]; pm[1] = nx1.mm[1];
                pmk[0] = mk[0]; pmk[1] = mk[1];
                cur = nx1;
                nx1 = nx2;
            }
            if (pmk[0]) flag_clr(pm[0]);
            if (pmk[1]) flag_clr(pm[1]);
        }
        wave_lds_fence(); /* (the flags are left clean for the wave's next hmm) */
    }
}

hipError_t mrp_launch_prune(const MrpBatchDev &d, const CrossCol *ccols_dev, const PruneHmm *hmms_dev, int64_t n_hmms, PruneParams p,
                            PruneScratch s, hipStream_t stream, LaunchCensus *census) {
    if (n_hmms <= 0) return hipSuccess;
    /* what the bin-streaming waves hold per column decides the instantiation (prune_class, mrp_level_order.h) */
    const PruneClass cls = prune_class(p.pairs, p.max_cells);
    if (p.S > MRP_PRUNE_MAX_S || cls == PRUNE_TOO_LARGE || p.max_merge > MRP_PRUNE_MAX_CELLS || p.n_bins > 1024) return hipErrorInvalidValue;
    /* once per device (thread-safe: the concurrent halves of a call launch from two host threads) */
    static PerDeviceOnce once;
    const hipError_t configured = once.run([] {
        hipError_t e = hipSuccess;
        auto big_lds = [&](const void *f) { if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); };
        big_lds((const void *) mrp_prune_kernel<512, 32, 2, 1, false>); big_lds((const void *) mrp_prune_kernel<512, 32, 2, 1, true>);
        big_lds((const void *) mrp_prune_kernel<256, 4, 1, 1, false>); big_lds((const void *) mrp_prune_kernel<256, 4, 1, 1, true>);
        big_lds((const void *) mrp_prune_kernel<512, 10, 1, 4, false>); big_lds((const void *) mrp_prune_kernel<512, 10, 1, 4, true>);
        big_lds((const void *) mrp_prune_kernel<512, 10, 2, 4, false>); big_lds((const void *) mrp_prune_kernel<512, 10, 2, 4, true>);
        big_lds((const void *) mrp_prune_kernel<1024, 36, 2, 1, false>); big_lds((const void *) mrp_prune_kernel<1024, 36, 2, 1, true>);
        return e;
    });
    if (configured != hipSuccess) return configured;
    const size_t lds = prune_lds_bytes(p.pairs, p.max_cells, p.max_merge); /* (mrp_level_order.h; within the budget at every reachable level) */
    if (lds > (size_t) MRP_LDS_BUDGET) return hipErrorInvalidValue;
    const dim3 grid((unsigned) (n_hmms < 65536 ? n_hmms : 65536));
    const PruneIn in{d.scols, ccols_dev, d.cell_f32, d.cell_b32, d.merge_f32, d.merge_b32, d.hmm_fb};
    /* The bin-streaming waves hold a column's f and b in registers: two groups of 2 waves x 32 cells per lane at 512 threads;
     * one group of 4 waves x 40 cells per lane (16-byte loads) at 512 threads for columns of up to 10 240 cells -- the
     * 100 x 100 cells of the shipped parameters: half the waves and 77 KB of LDS let two workgroups share a CU where the
     * 1 024-thread variant (two groups of 6 waves x 36 cells) fills it alone.  That variant holds up to 13 824 cells
     * (MRP_PRUNE_MAX_CELLS); the largest bound a level can have is 116 x 116 = 13 456 (MRP_PRUNE_MAX_S), so 13 457..13 824 is
     * covered only by the CPU check of the selector (tests/level_order_check.cpp), never by a launch.
     * p.pairs (includeInvertedPartitions and even column limits): the chain runs on complement pairs. */
    const bool pairs = p.pairs != 0;
#define PRUNE_LAUNCH(T_, CPT_, NGRP_, VEC_)                                                                                               \
    do {                                                                                                                                  \
        if (pairs) hipLaunchKernelGGL((mrp_prune_kernel<T_, CPT_, NGRP_, VEC_, true>), grid, dim3(T_), lds, stream, in, hmms_dev, n_hmms, p, s);  \
        else hipLaunchKernelGGL((mrp_prune_kernel<T_, CPT_, NGRP_, VEC_, false>), grid, dim3(T_), lds, stream, in, hmms_dev, n_hmms, p, s);       \
    } while (0)
    if (census) census->bump(census_prune_slot(cls, p.pairs));
    switch (cls) {
    /* columns of at most 256 entries (the first merge levels: a few reads per hmm): four waves, the table wave writes the bins */
    case PRUNE_256: PRUNE_LAUNCH(256, 4, 1, 1); break;
    case PRUNE_512X32: PRUNE_LAUNCH(512, 32, 2, 1); break;
    /* up to 5 120 entries -- the unit levels of the shipped parameters (100 x 100 cells = 5 000 units): the same four streaming waves as
     * two groups that alternate over the columns, so that a column's f and b have TWO column times to arrive (one group: 1 ms per
     * step slower) */
    case PRUNE_512X10_TWO_GROUPS: PRUNE_LAUNCH(512, 10, 2, 4); break;
    case PRUNE_512X10_ONE_GROUP: PRUNE_LAUNCH(512, 10, 1, 4); break;
    default: PRUNE_LAUNCH(1024, 36, 2, 1); break;
    }
#undef PRUNE_LAUNCH
    {
        const hipError_t fe = hipGetLastError();
        if (fe != hipSuccess) return fe;
    }
    {   /* the backward pass: one wave per hmm, four to a workgroup */
        const size_t back_lds = (size_t) 4 * ((size_t) (((p.max_merge + 127) >> 7) << 2)) * sizeof(uint32_t);
        const int64_t wgs = (n_hmms + 3) / 4;
        const dim3 bgrid((unsigned) (wgs < 65536 ? wgs : 65536));
        if (census) census->bump(pairs ? CENSUS_PRUNE_BACK_PAIRS : CENSUS_PRUNE_BACK_GENERAL);
        if (pairs) hipLaunchKernelGGL((mrp_prune_back_kernel<true>), bgrid, dim3(256), back_lds, stream, hmms_dev, n_hmms, p, s);
        else hipLaunchKernelGGL((mrp_prune_back_kernel<false>), bgrid, dim3(256), back_lds, stream, hmms_dev, n_hmms, p, s);
    }
    return hipGetLastError();
}
