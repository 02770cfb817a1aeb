/*
 * mrp_prune_feed.h -- the waves of mrp_prune_kernel (mrp_engine_kernels.hip) that feed the chain: wave 3 (the column's descriptor and the
 * parents' inverted transition tables, a column ahead; it also wipes the histograms) and waves 4.. (the posterior bins of whole
 * columns, streamed from f and b).  Each role runs its own loop over the columns and passes the barriers every role passes: one after
 * the prologue, one per column, one behind the last column (the chain on pairs: two).
 */
#ifndef MRP_PRUNE_FEED_H_
#define MRP_PRUNE_FEED_H_

#include "mrp_prune_ctx.h"
#include "mrp_prune_rule.h"

/* wave 3: the parents' transitions of the column after next.  Three columns are in the pipe: the tables of column
 * t are built from the registers while the transitions of column t + 1 and the descriptor of column t + 2 are in
 * flight.  The descriptors come by VECTOR loads (lane l = dword l of the CrossCol, lanes 16.. = the SweepCol) and
 * are taken apart with v_readlane a step later: a scalar load shares lgkmcnt with the LDS traffic of the table
 * build, and a wave that first has to wait for its descriptor before it can ask for the transitions it points to
 * pays two memory latencies per column -- with the chain on complement pairs this wave had become the slowest role. */
template <class Ctx>
static __device__ __forceinline__ void prune_role_tables(const Ctx &cx) {
    constexpr int W = Ctx::W, CPT = Ctx::CPT;
    constexpr bool PAIRS = Ctx::PAIRS;
    const PruneIn &d = cx.d;
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const PruneHmm &h = cx.h;
    const int K = cx.K, nb = cx.nb, lane = cx.lane, cap_c = cx.lds.cap_c;
    const int32_t total = cx.total;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    const bool units = cx.units;
    int &errbits = cx.errbits;
    uint32_t *const sh = cx.lds.sh, *const hist = cx.lds.hist, *const tab = cx.lds.tab;
    uint16_t *const bins = cx.lds.bins;
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
        uint32_t *t5[2] = {tA5, tA5 + PRUNE_TAB * PRUNE_SIDE};
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
            uint32_t *tb = tab + (tcol & 1) * 2 * PRUNE_TAB * PRUNE_SIDE;
            if (lane == 0) { /* the chain's view of the column (read after the barrier that ends this step) */
                uint32_t *col = sh + MB_COL + 4 * (tcol & 1);
                col[COL_DIMS] = (uint32_t) tcc.C2 | ((uint32_t) tcc.Mb << 16);
                col[COL_FLAGS] = (uint32_t) tcc.flags | ((tcc.a_part && tcc.d1 > 0) ? 0x100u : 0u) | ((tcc.b_part && tcc.d2 > 0) ? 0x200u : 0u) |
                         ((uint32_t) tcc.Pb << 16);
                if (PAIRS) { /* what the chain on pairs derives from these flags, as bits (see its unit() / parity() rule) */
                    const bool a_cp = tcc.a_part && tcc.d1 > 0, b_cp = tcc.b_part && tcc.d2 > 0;
                    const bool o_a = (tcc.flags & MRP_XF_OUT_A_PAIRED) != 0, o_b = (tcc.flags & MRP_XF_OUT_B_PAIRED) != 0;
                    const bool i_a = (tcc.flags & MRP_XF_IN_A_PAIRED) != 0, i_b = (tcc.flags & MRP_XF_IN_B_PAIRED) != 0;
                    col[COL_PAIRING] = ((a_cp && b_cp) ? 1u : 0u) | ((!a_cp && b_cp) ? 2u : 0u) | (a_cp ? 4u : 0u) | ((o_a && o_b) ? 8u : 0u) |
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
        uint32_t *hn = hist + ((k + 1) & 1) * PRUNE_HIST;
        if (!PAIRS || sh[MB_HIST_USED + ((k + 1) & 1)] != 0u) { /* (the chain on pairs says when it has used a histogram: one column in a hundred) */
            for (int i = lane; i < PRUNE_HIST; i += WAVE) hn[i] = 0u;
            if (PAIRS && lane == 0) sh[MB_HIST_USED + ((k + 1) & 1)] = 0u;
        }
        ROLE_BARRIER();
    }
    ROLE_CLK_DONE(3);
    lds_barrier();
    if (PAIRS) lds_barrier();
}

/* bins groups (waves 4..): group g handles the columns g, g + 2, ...  A step of its loop stores the bins of the
 * column whose f and b sit in the registers and requests the column after next into the same registers; the
 * group is idle during the other group's step.  Loads are issued for every register slot whatever the column's
 * size (beyond the column -- and beyond the last column -- the buffer descriptor's range check returns 0 without
 * touching memory): a load under a condition would make every slot a loop-carried merge of old and new value,
 * which costs a second register set.
 * The waves form NGRP groups (2: alternating over the columns, a column's f and b sit in a group's registers for two column times; 1:
 * one group, requested one column ahead) and hold CPT loads of VEC cells per lane and array. */
template <class Ctx>
static __device__ __forceinline__ void prune_role_bins(const Ctx &cx) {
    constexpr int CPT = Ctx::CPT, NGRP = Ctx::NGRP, VEC = Ctx::VEC, LG = Ctx::LG;
    constexpr bool PAIRS = Ctx::PAIRS;
    const PruneIn &d = cx.d;
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const PruneHmm &h = cx.h;
    const int K = cx.K, nb = cx.nb, wave = cx.wave, lane = cx.lane, cap_c = cx.lds.cap_c;
    const int32_t total = cx.total;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    const bool units = cx.units;
    int &errbits = cx.errbits;
    uint16_t *const bins = cx.lds.bins;
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

#endif
