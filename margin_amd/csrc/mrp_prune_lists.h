/*
 * mrp_prune_lists.h -- waves 1 and 2 of mrp_prune_kernel (mrp_engine_kernels.hip): the sorted lists of a finished selection, in two stages
 * one column apart.  Nothing later in the forward pass reads them: the next column's kept merge cells were already listed by wave 0
 * from the unsorted selection.
 *   Stage 1 (wave 1, column kk from selection buffer kk & 1): stable sort of the kept cells, kept lists to HBM, the posterior bins of
 *           the merge cells they lead to; leaves next | prev and that bin per sorted kept cell in LDS.
 *   Stage 2 (wave 2, one column later): distinct next merge cells in order of first use, stable sort by posterior, kept merge list
 *           to HBM.
 * Each role runs its own loop over the columns and passes the barriers every role passes: one after the prologue, one per column, one
 * behind the last column (the chain on pairs: two, its list stages run three columns deep).
 */
#ifndef MRP_PRUNE_LISTS_H_
#define MRP_PRUNE_LISTS_H_

#include "mrp_prune_ctx.h"
#include "mrp_prune_rule.h"

/* stage 1 under the general chain */
template <class Ctx>
static __device__ __forceinline__ void prune_lists_stage1(const Ctx &cx, int kk, int64_t mcell_off) {
    const PruneIn &d = cx.d;
    const PruneScratch &sc = cx.sc;
    const PruneHmm &h = cx.h;
    const int K = cx.K, S = cx.S, nb = cx.nb, lane = cx.lane;
    const int32_t total = cx.total;
    int &errbits = cx.errbits;
    uint32_t *const sel = cx.lds.sel, *const um = cx.lds.um, *const s1 = cx.lds.s1, *const sh = cx.lds.sh;
    const int b = kk & 1;
    const uint32_t *skey = sel + b * 2 * PRUNE_SP, *snp_in = skey + PRUNE_SP;
    uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
    const int n = (int) sh[MB_SEL_N + b];
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
    if (lane == 0) { sc.n_kept[lcol] = n; sh[MB_S1_N + b] = (uint32_t) n; }
}

/* The chain on pairs: stage 1 in two halves a column apart -- the posteriors of the merge cells are a gather from HBM (two microseconds
 * under load, as long as a whole column of the chain on pairs): asked for when the selection of column kk is read (step
 * kk + 1), used a step later, with the selection in registers meanwhile (the chain reuses its buffer).  The selection holds UNITS, at
 * most 64; a unit's two cells tie and are neighbours in list order, so the sorted units, each expanded to (cell 2u, cell 2u + 1), are
 * the sorted cells. */
struct PruneStage1Asked {
    uint32_t key = 0xFFFFFFFFu, np = 0u, fl = 0u;
    int32_t mf = 0, mb = 0;
    int n = 0;
};
template <class Ctx>
static __device__ __forceinline__ void prune_stage1_ask(const Ctx &cx, PruneStage1Asked &a, int kk, int64_t mcell_off) {
    const PruneIn &d = cx.d;
    const int K = cx.K, lane = cx.lane;
    const bool units = cx.units;
    const uint32_t *const sel = cx.lds.sel, *const sh = cx.lds.sh;
    const int b = kk & 1;
    const uint2 *selb = reinterpret_cast<const uint2 *>(sel) + b * 64; /* (bin << 14 | unit, next | prev << 16) */
    a.n = (int) sh[MB_SEL_N + b];
    a.fl = sh[MB_SEL_PAIRED + b]; /* bit 0: the column's cells come in pairs, 1: the merge cells after it, 2: those before it */
    const uint2 mine = selb[lane];
    a.key = lane < a.n ? (mine.x << 7) | (uint32_t) lane : 0xFFFFFFFFu; /* bin (10) | unit (14) | slot (7) */
    a.np = mine.y;
    a.mf = 0; a.mb = 0;
    if (kk + 1 < K && lane < a.n) {
        const uint32_t m = (mine.y & 0xFFFFu) >> (units ? (a.fl >> 1) & 1u : 0u); /* (units: the merge arrays hold merge units) */
        a.mf = d.merge_f32[mcell_off + m];
        a.mb = d.merge_b32[mcell_off + m];
    }
}
template <class Ctx>
static __device__ __forceinline__ void prune_stage1_finish(const Ctx &cx, const PruneStage1Asked &a, int kk) {
    const PruneScratch &sc = cx.sc;
    const PruneHmm &h = cx.h;
    const int K = cx.K, S = cx.S, nb = cx.nb, lane = cx.lane;
    const int32_t total = cx.total;
    int &errbits = cx.errbits;
    uint32_t *const s1 = cx.lds.s1, *const sh = cx.lds.sh;
    const int b = kk & 1;
    uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
    const int n = a.n;
    const uint32_t fl = a.fl, o_pm = (fl >> 1) & 1u, i_pm = (fl >> 2) & 1u;
    const int64_t lcol = h.col0 + kk;
    const bool has_merge = kk + 1 < K;
    uint32_t key[1] = {a.key};
    wave_bitonic_sort_n<1>(key, lane);
    const uint32_t mbin = has_merge && lane < n ? (uint32_t) posterior_bin(a.mf, a.mb, total, nb, &errbits) : 0u;
    /* what rides along with a unit comes from the lane that held it before the sort */
    const uint32_t src = key[0] & 0x3Fu, u = (key[0] >> 7) & 0x3FFFu;
    const uint32_t np_ = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (src << 2), (int) a.np);
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
    if (lane == 0) { sc.n_kept[lcol] = (fl & 1u) ? 2 * n : n; sh[MB_S1_N + b] = (uint32_t) n; sh[MB_S1_PAIRED + b] = fl; }
}

/* stage 2 under the chain on pairs */
template <class Ctx>
static __device__ __forceinline__ void prune_lists_stage2_pairs(const Ctx &cx, int kk) {
    const PruneScratch &sc = cx.sc;
    const PruneParams &p = cx.p;
    const PruneHmm &h = cx.h;
    const int K = cx.K, S = cx.S, lane = cx.lane;
    const int64_t hi_ = cx.hi_;
    int &errbits = cx.errbits;
    uint32_t *const s1 = cx.lds.s1, *const sh = cx.lds.sh, *const htab_key = cx.lds.htab_key, *const htab_val = cx.lds.htab_val;
    const int b = kk & 1;
    const uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
    const int n = (int) sh[MB_S1_N + b];
    const uint32_t o_pm = (sh[MB_S1_PAIRED + b] >> 1) & 1u;
    const int64_t lcol = h.col0 + kk;
    int mn_out = 0;
    if (kk + 1 < K) {
        /* distinct next merge UNITS in order of first use; the two merge cells of a unit enter the list in the order the
         * unit's first user reaches them: its even cell first (bit q of that cell's merge cell index), then its twin */
        for (int i = lane; i < PRUNE_HTAB; i += WAVE) { htab_key[i] = 0xFFFFFFFFu; htab_val[i] = 0xFFFFFFFFu; }
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
                q = (q + 1) & (PRUNE_HTAB - 1);
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
}

/* stage 2 under the general chain */
template <class Ctx>
static __device__ __forceinline__ void prune_lists_stage2(const Ctx &cx, int kk) {
    const PruneScratch &sc = cx.sc;
    const PruneParams &p = cx.p;
    const PruneHmm &h = cx.h;
    const int K = cx.K, S = cx.S, lane = cx.lane;
    const int64_t hi_ = cx.hi_;
    int &errbits = cx.errbits;
    uint32_t *const s1 = cx.lds.s1, *const sh = cx.lds.sh, *const htab_key = cx.lds.htab_key, *const htab_val = cx.lds.htab_val;
    const int b = kk & 1;
    const uint32_t *snp = s1 + b * 2 * PRUNE_SP, *sbin = snp + PRUNE_SP;
    const int n = (int) sh[MB_S1_N + b];
    const int64_t lcol = h.col0 + kk;
    int mn = 0;
    if (kk + 1 < K) {
        /* getLinkedMergeCells :989-1004: distinct next merge cells in order of first use (sorted order of the
         * kept cells): an open-addressing table of PRUNE_HTAB slots, merge cell -> smallest sorted index that uses it */
        for (int i = lane; i < PRUNE_HTAB; i += WAVE) { htab_key[i] = 0xFFFFFFFFu; htab_val[i] = 0xFFFFFFFFu; }
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
                    q = (q + 1) & (PRUNE_HTAB - 1);
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
}

/* wave 1: stage 1 of column k - 1 at step k (the chain on pairs: asked for at step k, finished at step k + 1) */
template <class Ctx>
static __device__ __forceinline__ void prune_role_lists1(const Ctx &cx) {
    const PruneIn &d = cx.d;
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const PruneHmm &h = cx.h;
    const int K = cx.K;
    [[maybe_unused]] const int lane = cx.lane;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    int64_t mcell_prev = 0; /* first merge cell of the merge column after column k - 1 */
    SweepCol scur = k_load(d.scols + h.col0);
    lds_barrier();
    ROLE_CLK_INIT();
    if constexpr (Ctx::PAIRS) {
        PruneStage1Asked asked;
        for (int k = 0; k < K; k++) {
            if (k > 1) prune_stage1_finish(cx, asked, k - 2);
            if (k > 0) prune_stage1_ask(cx, asked, k - 1, mcell_prev);
            mcell_prev = scur.mcell_off;
            if (k + 1 < K) scur = k_load(d.scols + h.col0 + k + 1);
            ROLE_BARRIER();
        }
        ROLE_CLK_DONE(1);
        if (K > 1) prune_stage1_finish(cx, asked, K - 2);
        prune_stage1_ask(cx, asked, K - 1, mcell_prev);
        lds_barrier();
        prune_stage1_finish(cx, asked, K - 1);
        lds_barrier();
    } else {
        for (int k = 0; k < K; k++) {
            if (k > 0) prune_lists_stage1(cx, k - 1, mcell_prev);
            mcell_prev = scur.mcell_off;
            if (k + 1 < K) scur = k_load(d.scols + h.col0 + k + 1);
            ROLE_BARRIER();
        }
        ROLE_CLK_DONE(1);
        prune_lists_stage1(cx, K - 1, mcell_prev);
        lds_barrier();
    }
}

/* wave 2: stage 2 of column k - 2 at step k; under the chain on pairs a column later, stage 1 takes two steps */
template <class Ctx>
static __device__ __forceinline__ void prune_role_lists2(const Ctx &cx) {
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const int K = cx.K;
    [[maybe_unused]] const int lane = cx.lane;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    lds_barrier();
    ROLE_CLK_INIT();
    if constexpr (Ctx::PAIRS) {
        for (int k = 0; k < K; k++) {
            if (k > 2) prune_lists_stage2_pairs(cx, k - 3);
            ROLE_BARRIER();
        }
        ROLE_CLK_DONE(2);
        if (K > 2) prune_lists_stage2_pairs(cx, K - 3);
        lds_barrier();
        if (K > 1) prune_lists_stage2_pairs(cx, K - 2);
        lds_barrier();
        prune_lists_stage2_pairs(cx, K - 1);
    } else {
        for (int k = 0; k < K; k++) {
            if (k > 1) prune_lists_stage2(cx, k - 2);
            ROLE_BARRIER();
        }
        ROLE_CLK_DONE(2);
        if (K > 1) prune_lists_stage2(cx, K - 2);
        lds_barrier();
        prune_lists_stage2(cx, K - 1);
    }
}

#endif
