/*
 * mrp_prune_chain_general.h -- wave 0 of mrp_prune_kernel (mrp_engine_kernels.hip), the general chain: the sequential walk over the
 * columns, without a barrier inside a column: kept merge cells -> candidates (64 per slot, as many slots as the column needs; cell
 * index by the closed form of the cross product order) -> posterior bins (LDS gathers) -> cutoff bin by histogram -> selection (ties
 * in the cutoff bin by list order = cell index, ranked through a bitmap) -> the distinct next merge cells of the selection = the kept
 * merge cells of the next column, listed with their per-side indices.  (The chain on complement pairs: mrp_prune_chain_pairs.h.)
 */
#ifndef MRP_PRUNE_CHAIN_GENERAL_H_
#define MRP_PRUNE_CHAIN_GENERAL_H_

#include "mrp_cross_cells.h"
#include "mrp_prune_ctx.h"
#include "mrp_prune_rule.h"

template <class Ctx>
static __device__ __forceinline__ void prune_role_chain_general(const Ctx &cx) {
    [[maybe_unused]] const PruneScratch &sc = cx.sc;
    const PruneParams &p = cx.p;
    const int K = cx.K, nb = cx.nb, lane = cx.lane, cap_c = cx.lds.cap_c;
    [[maybe_unused]] const int64_t hi_ = cx.hi_;
    uint32_t *const sel = cx.lds.sel, *const sh = cx.lds.sh, *const hist = cx.lds.hist, *const bmp_c = cx.lds.bmp_c, *const bmp_m = cx.lds.bmp_m;
    uint32_t *const kml = cx.lds.kml, *const minfo = cx.lds.minfo, *const heads = cx.lds.heads, *const pref = cx.lds.pref;
    const uint32_t *const tab = cx.lds.tab;
    const uint16_t *const bins = cx.lds.bins;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
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
    for (int k = 0; k < K; k++) {
        SEC(7);
        const int b = k & 1;
        /* what the chain needs of the column's CrossCol comes through LDS from the table wave (MB_COL): a scalar
         * load here would sit in the same counter as the LDS traffic, and every LDS wait of the column would wait for it */
        const uint32_t cd0 = sh[MB_COL + 4 * b + COL_DIMS], cd1 = sh[MB_COL + 4 * b + COL_FLAGS];
        uint32_t *skey = sel + b * 2 * PRUNE_SP, *snp = skey + PRUNE_SP;
        const uint32_t *tA = tab + b * 2 * PRUNE_TAB * PRUNE_SIDE, *tB = tA + PRUNE_TAB * PRUNE_SIDE;
        const uint32_t *cntA = tA, *startA = tA + 128, *listA = tA + 256, *nxA = tA + 384;
        const uint32_t *cntB = tB, *startB = tB + 128, *listB = tB + 256, *nxB = tB + 384;
        const uint16_t *bin_k = bins + b * cap_c;
        uint32_t *hk = hist + b * PRUNE_HIST;
        uint32_t *kmn = kml + (b ^ 1) * PRUNE_SP; /* the kept merge cells leading into column k + 1 */
        const uint32_t cflags = cd1 & 0xFFu;
        const bool inv = (cflags & MRP_XF_INVERTED) != 0;
        const uint32_t C2 = (cd0 & 0xFFFFu) > 128u ? 128u : (cd0 & 0xFFFFu), Mb = cd0 >> 16;
        const bool a_cp = inv && (cd1 & 0x100u), b_cp = inv && (cd1 & 0x200u);
        const bool out_ap = (cflags & MRP_XF_OUT_A_PAIRED) != 0, out_bp = (cflags & MRP_XF_OUT_B_PAIRED) != 0;
        const bool has_next = k + 1 < K;
        const int nkm = (int) sh[MB_KML_N + b];
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
                    first = (atomicOr(&bmp_m[(nxt >> 5) & (PRUNE_BMP - 1)], bit) & bit) == 0u;
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
            const PruneCutoff cut = prune_cutoff(hk, lane, p.thr_bin, thr_all, L, [&](int g) { return kept_count(L, g, p.min_p, p.max_p); });
            n = cut.n;
            const int B = cut.B, quota = cut.quota;
            const int nG = n - quota;
            const bool whole_bin = cut.in_B == quota; /* the cutoff bin is kept entirely: no ranking needed */
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
                 * of marks below it */
                prune_bitmap_prefix(bmp_c, pref, lane);
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
        if (lane == 0) { sh[MB_SEL_N + b] = (uint32_t) n; sh[MB_KML_N + (b ^ 1)] = (uint32_t) cm; }
        /* the marks of the next merge cells go */
        if (has_next) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int idx = lane + u * WAVE;
                if (idx < cm) bmp_m[((kmn[idx] & 0x3FFFu) >> 5) & (PRUNE_BMP - 1)] = 0u;
            }
        }
        SEC(6);
        ROLE_BARRIER();
    }
    ROLE_CLK_DONE(0);
    SEC_DONE();
    lds_barrier();
}

#endif
