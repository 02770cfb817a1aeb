/*
 * mrp_prune_lds.h -- the dynamic LDS of the prune kernels (mrp_engine_kernels.hip): the regions of mrp_prune_kernel's workgroup, defined
 * once for the host's size (prune_lds_bytes) and the kernel's pointers (prune_lds_carve); the mailboxes through which its roles talk; the
 * flag words of mrp_prune_back_kernel.  No HIP call: mrp_level_order.h includes it and tests/level_order_check.cpp compiles it on the CPU.
 */
#ifndef MRP_PRUNE_LDS_H_
#define MRP_PRUNE_LDS_H_

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define MRP_HD __host__ __device__
#else
#define MRP_HD
#endif

#define PRUNE_SP 128    /* slots of the selection buffers (S <= MRP_PRUNE_MAX_S) */
#define PRUNE_TAB 5     /* tables per side and buffer: cnt, start, list, nx, pv, PRUNE_SIDE entries each */
#define PRUNE_HIST 1024 /* bins of a histogram, 16 per lane of the cutoff search: bin b lives at (b & 15) * 64 + (b >> 4) */
#define PRUNE_SIDE 128  /* entries of one table of one side: a parent's column has at most 128 cells */
#define PRUNE_BMP 512   /* words of a bitmap over a column's cells or merge cells (16 384 bits); also the prefix counts, one per word */
#define PRUNE_CHUNK 512 /* candidates of one chunk of the general chain: eight slots of 64, one range mark each */
#define PRUNE_HTAB 256  /* slots of the merge-cell hash (at most PRUNE_SP keys) */

/* kept flag per merge cell (the backward pass, one set per wave): words, a multiple of four */
MRP_HD constexpr int prune_flag_words(int max_merge) { return ((max_merge + 127) >> 7) << 2; }

/* posterior bins of one column: one per cell; where the chain runs on complement pairs one per unit (cells 2u, 2u + 1 tie) */
MRP_HD constexpr int prune_bins_cap(bool pairs, int max_cells) { return pairs ? ((max_cells + 1) / 2 + 3) & ~3 : (max_cells + 3) & ~3; }

/* The regions in their order, as dword offsets from the start of the workgroup's LDS.  (wave n: the role, mrp_prune_kernel) */
struct PruneLdsOff {
    int sel;       /* [2][2][SP] selection of column k in buffer k & 1: key = bin << 14 | cell, np = next | prev << 16 (pairs: [2][64] uint2) */
    int um;        /* [SP] posterior bin of the merge cell each selected cell leads to (selection order); wave 1 */
    int s1;        /* [2][2][SP] stage 1 -> stage 2: next | prev and merge posterior bin per sorted kept cell */
    int sh;        /* [64] the mailboxes (PruneMailbox) */
    int hist;      /* [2][PRUNE_HIST] */
    int bmp_c;     /* [PRUNE_BMP] cells of the cutoff bin, by cell index */
    int bmp_m;     /* [PRUNE_BMP] next merge cells seen (directly behind bmp_c: the two are cleared as one) */
    int kml;       /* [2][SP] kept merge cells leading into column k, buffer k & 1 */
    int minfo;     /* [SP][2] per kept merge cell: what its candidates need (wave 0; pairs: [64] uint4) */
    int heads;     /* [PRUNE_CHUNK] "a range starts here" marks of one chunk of candidates, zero between uses (wave 0) */
    int pref;      /* [PRUNE_BMP] marks before each word of the cutoff bin's bitmap (wave 0) */
    int tab;       /* [2 buffers][2 sides][PRUNE_TAB][PRUNE_SIDE] */
    int htab_key;  /* [PRUNE_HTAB] merge cell -> first kept cell that uses it (open addressing); wave 2 */
    int htab_val;  /* [PRUNE_HTAB] */
    int bins;      /* [2][cap_c] 16-bit posterior bin per cell */
    int cap_c;     /* prune_bins_cap: entries of one column of bins */
    int end;       /* behind the last region */
};
MRP_HD constexpr PruneLdsOff prune_lds_offsets(bool pairs, int max_cells) {
    PruneLdsOff o{};
    int at = 0;
    o.sel = at;      at += 4 * PRUNE_SP;
    o.um = at;       at += PRUNE_SP;
    o.s1 = at;       at += 4 * PRUNE_SP;
    o.sh = at;       at += 64;
    o.hist = at;     at += 2 * PRUNE_HIST;
    o.bmp_c = at;    at += PRUNE_BMP;
    o.bmp_m = at;    at += PRUNE_BMP;
    o.kml = at;      at += 2 * PRUNE_SP;
    o.minfo = at;    at += 2 * PRUNE_SP;
    o.heads = at;    at += PRUNE_CHUNK;
    o.pref = at;     at += PRUNE_BMP;
    o.tab = at;      at += 2 * 2 * PRUNE_TAB * PRUNE_SIDE;
    o.htab_key = at; at += PRUNE_HTAB;
    o.htab_val = at; at += PRUNE_HTAB;
    o.cap_c = prune_bins_cap(pairs, max_cells);
    o.bins = at;     at += 2 * o.cap_c / 2; /* (two columns of 16-bit entries; cap_c is a multiple of four) */
    o.end = at;
    return o;
}
/* the request is this much larger than the regions (it always was: kept) */
#define PRUNE_LDS_TAIL_SLACK 16
static inline size_t prune_lds_bytes(int pairs, int max_cells) { return (size_t) prune_lds_offsets(pairs != 0, max_cells).end * 4 + PRUNE_LDS_TAIL_SLACK; }

/* The mailboxes: slots of sh[], each written by one wave and read by another a column or more later (the column barrier lies between).
 * A slot `+ b` has two entries, for the columns k with k & 1 = b.  Step k: the barrier interval in which the chain works on column k. */
enum PruneMailbox {
    /* selected cells (pairs: units) of column k.  Wave 0 at step k -> wave 1 at step k + 1 (lists_stage1 / stage1_ask of column k) */
    MB_SEL_N = 32,
    /* sorted kept cells (pairs: units) of column k in s1.  Wave 1, stage 1 of column k (general: step k + 1; pairs: stage1_finish at step
     * k + 2) -> wave 2, lists_stage2 of column k one step later */
    MB_S1_N = 36,
    /* kept merge cells (pairs: units) leading into column k, in kml.  Wave 0 at step k - 1 (the prologue for column 0) -> wave 0 at step k */
    MB_KML_N = 40,
    /* pairs: bit 0 the cells of column k come in pairs, 1 the merge cells behind it do, 2 those before it.  Wave 0 at step k -> wave 1,
     * stage1_ask of column k at step k + 1 */
    MB_SEL_PAIRED = 44,
    /* pairs: the same bits beside the stage-1 buffer.  Wave 1, stage1_finish of column k at step k + 2 -> wave 2, lists_stage2 at step k + 3 */
    MB_S1_PAIRED = 46,
    /* the chain's view of column k's CrossCol, four dwords at + 4 b (16-byte aligned: the chain on pairs reads a uint4), PruneColWord.
     * Wave 3 at step k - 1 (the prologue for column 0) -> wave 0 at step k */
    MB_COL = 48,
    /* pairs: the chain used histogram b at column k.  Wave 0 at step k -> wave 3 at step k + 1, which wipes it for column k + 2 and clears
     * the slot */
    MB_HIST_USED = 56,
};
/* the dwords of a column's mailbox (the fourth is unused) */
enum PruneColWord {
    COL_DIMS = 0,   /* C2 | Mb << 16 */
    COL_FLAGS = 1,  /* CrossCol.flags | a_cp << 8 | b_cp << 9 | Pb << 16 */
    COL_PAIRING = 2 /* pairs: the unit / parity bits the chain on pairs works with (prune_role_tables writes them, prune_role_chain_pairs names them) */
};

/* What the kernel relies on, at sizes on both sides of a multiple of four cells, for both kinds of bins (the regions before the bins
 * do not depend on the sizes; tests/level_order_check.cpp sweeps the sizes). */
constexpr bool prune_lds_aligned(bool pairs, int max_cells) {
    const PruneLdsOff o = prune_lds_offsets(pairs, max_cells);
    return o.sel % 2 == 0 && o.s1 % 2 == 0        /* sel and s1 are read as uint2 */
           && o.minfo % 4 == 0                    /* minfo is read as uint4 (the records of the chain on pairs) */
           && (o.sh + MB_COL) % 4 == 0            /* a column's mailbox is read as uint4 */
           && o.bins % 4 == 0 && o.cap_c % 4 == 0 /* the first column of bins starts on 16 bytes, the second on 8: written as dwords and uint2 */
           && o.bmp_m == o.bmp_c + PRUNE_BMP;     /* the two bitmaps are cleared as one */
}
static_assert(prune_lds_aligned(false, 1) && prune_lds_aligned(true, 1) && prune_lds_aligned(false, 13453) && prune_lds_aligned(true, 13455),
              "alignment of the prune kernel's LDS regions");

/* the kernel's pointers (base: 16-byte aligned, as dynamic LDS is) */
struct PruneLds {
    uint32_t *sel, *um, *s1, *sh, *hist, *bmp_c, *bmp_m, *kml, *minfo, *heads, *pref, *tab, *htab_key, *htab_val;
    uint16_t *bins;
    int cap_c;
};
MRP_HD inline PruneLds prune_lds_carve(uint32_t *base, bool pairs, int max_cells) {
    const PruneLdsOff o = prune_lds_offsets(pairs, max_cells);
    return PruneLds{base + o.sel, base + o.um, base + o.s1, base + o.sh, base + o.hist, base + o.bmp_c, base + o.bmp_m, base + o.kml, base + o.minfo,
                    base + o.heads, base + o.pref, base + o.tab, base + o.htab_key, base + o.htab_val, reinterpret_cast<uint16_t *>(base + o.bins),
                    o.cap_c};
}

#endif
