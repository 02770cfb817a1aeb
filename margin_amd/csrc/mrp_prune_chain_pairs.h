/*
 * mrp_prune_chain_pairs.h -- wave 0 of mrp_prune_kernel (mrp_engine_kernels.hip) where the chain runs on complement PAIRS
 * (includeInvertedPartitions, even column limits): the sequential walk over the columns, without a barrier inside a column.
 *
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
 * dropped.
 *
 * One slot of 64 candidates at a time, start to finish (owner, parent cells, unit, posterior bin, next merge unit):
 * the slots of a column are independent, but a column links 65 units on average -- one or two slots -- and code that
 * keeps eight slots in flight at once spends more instructions moving its register tuples through the "has this slot
 * work" branches than on the work.  Records of the kept merge units (16 bytes, with the reciprocal for the division
 * by the side-B count), the selection (key and transitions as one 8-byte entry) and the marks sit in LDS.
 */
#ifndef MRP_PRUNE_CHAIN_PAIRS_H_
#define MRP_PRUNE_CHAIN_PAIRS_H_

#include <type_traits>

#include "mrp_cross_cells.h"
#include "mrp_prune_ctx.h"
#include "mrp_prune_rule.h"

template <class Ctx>
static __device__ __forceinline__ void prune_role_chain_pairs(const Ctx &cx) {
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const PruneParams &p = cx.p;
    const int K = cx.K, nb = cx.nb, lane = cx.lane, cap_c = cx.lds.cap_c;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    int &errbits = cx.errbits;
    uint32_t *const sel = cx.lds.sel, *const sh = cx.lds.sh, *const hist = cx.lds.hist, *const bmp_c = cx.lds.bmp_c, *const bmp_m = cx.lds.bmp_m;
    uint32_t *const kml = cx.lds.kml, *const minfo = cx.lds.minfo, *const heads = cx.lds.heads, *const pref = cx.lds.pref;
    const uint32_t *const tab = cx.lds.tab;
    const uint16_t *const bins = cx.lds.bins;
    /* the chain wave goes first whenever it can issue: alone on the device that changes nothing (its SIMD's helper
     * waves are parked), beside the kernels of other batches on the same CU it is worth ~2 % of a call */
    __builtin_amdgcn_s_setprio(3);
    if (lane == 0) {
        kml[0] = 0u;   /* column 0: every cell is "linked" (one virtual merge cell in front of it) */
        sh[MB_KML_N] = 1u;
    }
    lds_barrier();
    ROLE_CLK_INIT();
    SEC_INIT();
    uint4 *rec = reinterpret_cast<uint4 *>(minfo);       /* [64] per kept merge unit of the column */
    for (int k = 0; k < K; k++) {
        SEC(7);
        const int b = k & 1;
        const uint4 cd = *reinterpret_cast<const uint4 *>(sh + MB_COL + 4 * b);
        const int nkm = (int) sh[MB_KML_N + b];
        const uint32_t ent_ = kml[b * PRUNE_SP + lane];
        const uint32_t cd0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.x), cd1 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.y);
        const uint32_t cd2 = (uint32_t) __builtin_amdgcn_readfirstlane((int) cd.z); /* the table wave's bits */
        uint2 *selb = reinterpret_cast<uint2 *>(sel) + b * 64; /* selection of column k: (bin << 14 | unit, next | prev << 16 of the unit's even cell) */
        const uint32_t *tA = tab + b * 2 * PRUNE_TAB * PRUNE_SIDE, *tB = tA + PRUNE_TAB * PRUNE_SIDE;
        const uint32_t *csA = tA + 128, *listA = tA + 256, *nxA = tA + 384;
        const uint32_t *csB = tB + 128, *listB = tB + 256, *nxB = tB + 384;
        const uint16_t *bin_k = bins + b * cap_c;
        uint32_t *hk = hist + b * PRUNE_HIST;
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
                    first = (atomicOr(&bmp_m[(mu2 >> 5) & (PRUNE_BMP - 1)], bit) & bit) == 0u;
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
                    if (has_next && take) old[j] = atomicOr(&bmp_m[(mu2[j] >> 5) & (PRUNE_BMP - 1)], 1u << (mu2[j] & 31u));
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
            if (lane == 0) sh[MB_HIST_USED + b] = 1u; /* the table wave wipes this histogram before its next use */
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
            const PruneCutoff cut = prune_cutoff(hk, lane, p.thr_bin, thr_all, Lu, kept_units);
            n = cut.n;
            const int B = cut.B, quota = cut.quota;
            const int nG = n - quota;
            const bool whole_bin = cut.in_B == quota; /* the cutoff bin is kept entirely: no ranking needed */
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
                prune_bitmap_prefix(bmp_c, pref, lane);
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
            sh[MB_SEL_N + b] = (uint32_t) n; sh[MB_KML_N + (b ^ 1)] = (uint32_t) cm;
            sh[MB_SEL_PAIRED + b] = (w_c == 2 ? 1u : 0u) | (o_pm << 1) | (i_pm << 2); /* for the list stages */
        }
        /* the marks of the next merge units go */
        if (has_next && lane < cm) bmp_m[((kmn[lane] & 0x3FFFu) >> 5) & (PRUNE_BMP - 1)] = 0u;
        SEC(6);
        ROLE_BARRIER();
    }
    ROLE_CLK_DONE(0);
    SEC_DONE();
    lds_barrier();
    lds_barrier(); /* (the list stages of the chain on pairs run three columns deep) */
}

#endif
