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
 *
 * The forward kernel's parts: mrp_prune_lds.h (its LDS layout and mailboxes), mrp_prune_ctx.h (the workgroup context a role takes),
 * and a function per role: mrp_prune_chain_pairs.h, mrp_prune_chain_general.h (wave 0), mrp_prune_lists.h (waves 1, 2),
 * mrp_prune_feed.h (wave 3, waves 4..).
 */
#include "mrp_engine.h"
#include "mrp_internal.h" /* PerDeviceOnce */
#include "mrp_level_order.h" /* prune_class, prune_lds_bytes */
#include "mrp_prune_chain_general.h"
#include "mrp_prune_chain_pairs.h"
#include "mrp_prune_feed.h"
#include "mrp_prune_lists.h"
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
 *
 * T threads; the bin-streaming waves (all but the first four) form NGRP groups and hold CPT loads of VEC cells per lane and array
 * (prune_role_bins).  Every role runs its own loop over the columns (the registers of one role are not live in the others); all of
 * them pass the same barriers: one after the prologue, one per column, one before the last merge list (the chain on pairs: two).
 */
template <int T, int CPT, int NGRP, int VEC, bool PAIRS>
__global__ void __launch_bounds__(T, T <= 512 ? 4 : 1) mrp_prune_kernel(PruneIn d, const PruneHmm *__restrict__ hmms, int64_t n_hmms,
                                                      PruneParams p, PruneScratch sc) {
    extern __shared__ uint32_t lds[];
    const int S = p.S;
    const int nb = p.n_bins;
    const bool units = PAIRS && p.pairs == 2; /* the level's f, b and merge arrays hold one entry per unit (MRP_XF_UNITS) */
    const PruneLds L = prune_lds_carve(lds, PAIRS, p.max_cells);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    /* The four role waves of a workgroup sit on the CU's four SIMDs (wave i on SIMD i mod 4).  Workgroups that share a CU
     * rotate the roles: otherwise every chain wave -- the one wave of a workgroup that is busy all the time -- would issue
     * from SIMD 0 and the workgroups would take turns on it. */
    const int hw_wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int wave = hw_wave < 4 ? ((hw_wave + (int) (blockIdx.x & 3u)) & 3) : hw_wave;

    for (int64_t hi_ = blockIdx.x; hi_ < n_hmms; hi_ += gridDim.x) {
        int errbits = 0;
        const PruneHmm h = k_load(hmms + hi_);
        const int32_t total = (int32_t) d.hmm_fb[2 * h.hmm_index]; /* max mode: the same integer for every column */
        for (int i = tid; i < 2 * PRUNE_HIST; i += T) L.hist[i] = 0;
        for (int i = tid; i < 2 * PRUNE_BMP; i += T) L.bmp_c[i] = 0; /* both bitmaps */
        for (int i = tid; i < PRUNE_CHUNK; i += T) L.heads[i] = 0;
        if (tid < 64) L.sh[tid] = 0u;
        __syncthreads();

        /* ---- stRPHmm_pruneForwards hmm.c:1049-1109 ---- */
        const PruneCtx<T, CPT, NGRP, VEC, PAIRS> cx{L, d, sc, p, h, h.n_cols, S, total, nb, wave, lane, hi_, units, errbits};
        if (wave == 0) {
            if constexpr (PAIRS) prune_role_chain_pairs(cx);
            else prune_role_chain_general(cx);
        } else if (wave == 1) prune_role_lists1(cx);
        else if (wave == 2) prune_role_lists2(cx);
        else if (wave == 3) prune_role_tables(cx);
        else prune_role_bins(cx);
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
    const int n_flagw = prune_flag_words(p.max_merge);
    uint32_t *flagw = lds + wave * n_flagw;             /* [max_merge bits] kept flag per merge cell, this wave's */
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
    const size_t lds = prune_lds_bytes(p.pairs, p.max_cells); /* (mrp_prune_lds.h; within the budget at every reachable level) */
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
        const size_t back_lds = (size_t) 4 * (size_t) prune_flag_words(p.max_merge) * sizeof(uint32_t);
        const int64_t wgs = (n_hmms + 3) / 4;
        const dim3 bgrid((unsigned) (wgs < 65536 ? wgs : 65536));
        if (census) census->bump(pairs ? CENSUS_PRUNE_BACK_PAIRS : CENSUS_PRUNE_BACK_GENERAL);
        if (pairs) hipLaunchKernelGGL((mrp_prune_back_kernel<true>), bgrid, dim3(256), back_lds, stream, hmms_dev, n_hmms, p, s);
        else hipLaunchKernelGGL((mrp_prune_back_kernel<false>), bgrid, dim3(256), back_lds, stream, hmms_dev, n_hmms, p, s);
    }
    return hipGetLastError();
}
