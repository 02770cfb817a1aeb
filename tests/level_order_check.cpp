/*
 * level_order_check.cpp -- the host arithmetic of staging a resident level (margin_amd/csrc/mrp_level_order.h) without a device:
 * the order and launch classes of random levels against a plain restatement, the prune kernel's class and the cross product + emission
 * plan on both sides of every threshold, the census slots, the block carver's two passes against each other, and the layout of a work
 * queue's chunk block.
 * Built and run by tests/test_level_order.py with the address and undefined-behaviour sanitizers; prints "level order ok".
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../margin_amd/csrc/mrp_level_order.h"

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const int32_t EDGES[] = {1, 2, 100, 2 * MRP_MINI_MAX_UNITS - 1, 2 * MRP_MINI_MAX_UNITS, 2 * MRP_MINI_MAX_UNITS + 1, 200, 255, 256, 257, 1000, 4095, 4096, 4097, 9000};
static const int N_EDGES = (int) (sizeof(EDGES) / sizeof(EDGES[0]));

/* mode 0: every class and the single-wave hmms mixed; 1, 2, 3: all hmms narrow / mid / wide (so that one class holds all n) */
static std::vector<mrp_xhmm> random_level(std::mt19937 &rng, int64_t n, int mode) {
    static const int32_t COLS[] = {1, 2, 3, 5, 8};
    std::vector<mrp_xhmm> x((size_t) n);
    for (auto &h : x) {
        h = mrp_xhmm{};
        h.n_cols = COLS[rng() % 5];
        h.bound_max_cells = mode == 0 ? EDGES[rng() % N_EDGES] : mode == 1 ? 129 + (int32_t) (rng() % 128) : 257 + (int32_t) (rng() % 5000);
        h.bound_max_merge = mode == 0 ? EDGES[rng() % N_EDGES] : mode == 3 ? 4097 + (int32_t) (rng() % 5000) : 1 + (int32_t) (rng() % 4096);
        h.bound_cells = (int64_t) (rng() % 40) * 3 + 1; /* few distinct values: ties; not multiples of 4: the sum pads */
        h.bound_merge = (int64_t) (rng() % 1000);
    }
    return x;
}

static void check_level(const std::vector<mrp_xhmm> &x, bool units) {
    const int64_t n = (int64_t) x.size();
    LevelOrder o;
    o.perm.assign(7, -1); o.wide.order.assign(3, -1); o.n_mini = 99; o.bound_cells = 5; /* a reused object: nothing of the level before stays */
    level_sort(x.data(), n, units, o);
    level_classes(x.data(), n, units, o);
    auto mini = [&](int32_t i) { return units && x[i].bound_max_cells <= 2 * MRP_MINI_MAX_UNITS && x[i].bound_max_merge <= 2 * MRP_MINI_MAX_UNITS; };

    /* perm is a permutation, pos its inverse */
    CHECK((int64_t) o.perm.size() == n && (int64_t) o.pos.size() == n);
    std::vector<char> seen((size_t) n, 0);
    for (int64_t j = 0; j < n; j++) {
        const int32_t i = o.perm[(size_t) j];
        CHECK(i >= 0 && i < n && !seen[(size_t) i]);
        seen[(size_t) i] = 1;
        CHECK(o.pos[(size_t) i] == j);
    }
    /* non-mini precede mini; each part in descending n_cols, equal n_cols in index order */
    int64_t n_mini = 0;
    for (int64_t i = 0; i < n; i++) n_mini += mini((int32_t) i);
    CHECK(o.n_mini == n_mini);
    for (int64_t j = 0; j < n; j++) CHECK(mini(o.perm[(size_t) j]) == (j >= n - n_mini));
    for (int64_t j = 1; j < n; j++) {
        if (j == n - n_mini) continue;
        const int32_t a = o.perm[(size_t) j - 1], b = o.perm[(size_t) j];
        CHECK(x[a].n_cols > x[b].n_cols || (x[a].n_cols == x[b].n_cols && a < b));
    }

    /* the classes partition the non-mini hmms by the two thresholds, wide / mid / narrow */
    std::vector<int32_t> want[3];
    int32_t max_cells = 1, max_merge = 1;
    int64_t bound_cells = 0, bound_merge = 0;
    for (int32_t i = 0; i < n; i++) {
        max_cells = std::max(max_cells, x[i].bound_max_cells);
        max_merge = std::max(max_merge, x[i].bound_max_merge);
        bound_cells += (x[i].bound_cells + 3) / 4 * 4;
        bound_merge += x[i].bound_merge;
        if (mini(i)) continue;
        want[x[i].bound_max_cells <= 256 ? 2 : x[i].bound_max_merge <= 4096 ? 1 : 0].push_back(i);
    }
    const LevelClass *got[3] = {&o.wide, &o.mid, &o.narrow};
    for (int c = 0; c < 3; c++) {
        /* up to 4 096 hmms: largest bound_cells first, equal ones in index order; more: index order */
        if (want[c].size() <= 4096)
            std::stable_sort(want[c].begin(), want[c].end(), [&](int32_t a, int32_t b) { return x[a].bound_cells > x[b].bound_cells; });
        CHECK(got[c]->order == want[c]);
        int m = 1;
        for (int32_t i : want[c]) m = std::max(m, x[i].bound_max_merge);
        CHECK(got[c]->max_merge == (units ? (m + 1) / 2 + 1 : m));
    }
    CHECK(o.max_cells == max_cells && o.max_merge == max_merge);
    CHECK(o.bound_cells == bound_cells && o.bound_merge == bound_merge);
}

/* The prune kernel's instantiation for (pairs, max_cells), restated as a table: the largest number of entries a class holds, by what
 * its bin-streaming waves keep in registers (waves x lanes x entries per lane).  A unit level (pairs == 2) holds one entry per
 * complement pair, half the cells rounded up.  More than 13 824 cells: no class, the launcher refuses. */
static int prune_class_restated(int pairs, int max_cells) {
    static const int HOLDS[5] = {256 /* 4 x 64 x 1 */, 4096 /* 2 x 64 x 32 */, 5120 /* 2 x 64 x 40 */, 10240 /* 4 x 64 x 40 */, 13824 /* 6 x 64 x 36 */};
    if (max_cells > 13824) return -1;
    const int held = pairs == 2 ? max_cells / 2 + max_cells % 2 : max_cells;
    for (int k = 0; k < 5; k++)
        if (held <= HOLDS[k]) return k;
    return -1;
}

static void check_prune_selector() {
    CHECK(PRUNE_256 == 0 && PRUNE_512X32 == 1 && PRUNE_512X10_TWO_GROUPS == 2 && PRUNE_512X10_ONE_GROUP == 3 && PRUNE_1024 == 4 && PRUNE_CLASSES == 5);
    CHECK(PRUNE_TOO_LARGE == -1 && MRP_PRUNE_MAX_CELLS == 13824 && MRP_PRUNE_MAX_S * MRP_PRUNE_MAX_S == 13456);
    /* both sides of every threshold, named: cell levels (general chain, pairs over per-cell arrays) ... */
    struct { int max_cells, want; } const CELL_EDGES[] = {{1, 0}, {256, 0}, {257, 1}, {4096, 1}, {4097, 2}, {5120, 2}, {5121, 3}, {10240, 3}, {10241, 4},
                                                          {13456, 4}, {13457, 4}, {13824, 4}, {13825, -1}};
    for (const auto &e : CELL_EDGES)
        for (int pairs = 0; pairs < 2; pairs++) CHECK((int) prune_class(pairs, e.max_cells) == e.want);
    /* ... and unit levels: held = (max_cells + 1) / 2, so a threshold t sits between 2 t and 2 t + 1 cells; the range still ends at
     * 13 824 CELLS (6 912 units: the 1 024-thread class is never reached on units) */
    struct { int max_cells, want; } const UNIT_EDGES[] = {{1, 0}, {511, 0}, {512, 0}, {513, 1}, {8191, 1}, {8192, 1}, {8193, 2}, {10239, 2}, {10240, 2}, {10241, 3},
                                                          {13456, 3}, {13824, 3}, {13825, -1}};
    for (const auto &e : UNIT_EDGES) CHECK((int) prune_class(2, e.max_cells) == e.want);
    /* every size against the restatement, every mode; the census slot is class-major, mode-minor and inside the prune block */
    for (int pairs = 0; pairs < 3; pairs++)
        for (int max_cells = 1; max_cells <= 13824 + 300; max_cells++) {
            const int want = prune_class_restated(pairs, max_cells);
            CHECK((int) prune_class(pairs, max_cells) == want);
            CHECK(prune_held(pairs, max_cells) == (pairs == 2 ? (max_cells + 1) / 2 : max_cells));
            if (want >= 0) {
                const int slot = census_prune_slot((PruneClass) want, pairs);
                CHECK(slot == CENSUS_PRUNE + 3 * want + pairs && slot >= CENSUS_PRUNE && slot < CENSUS_PRUNE_BACK_GENERAL);
            }
        }
}

/* The prune kernel's LDS request never exceeds the budget at a level the selector accepts (so the launcher's refusal for LDS is
 * unreachable): largest at the largest per-cell level under the general chain; monotone in the size; halved bins on pairs. */
static void check_prune_lds() {
    CHECK(prune_lds_bytes(0, 13456) == 89424);
    CHECK(prune_lds_bytes(0, MRP_PRUNE_MAX_CELLS) <= (size_t) MRP_LDS_BUDGET);
    for (int pairs = 0; pairs < 3; pairs++)
        for (int cells = 1; cells <= MRP_PRUNE_MAX_CELLS; cells += 97) {
            CHECK(prune_lds_bytes(pairs, cells) <= prune_lds_bytes(0, MRP_PRUNE_MAX_CELLS));
            CHECK(prune_lds_bytes(pairs, cells) <= prune_lds_bytes(pairs, cells + 1));
            CHECK(prune_lds_bytes(pairs, cells) % 4 == 0);
        }
    CHECK(prune_lds_bytes(1, 13456) == prune_lds_bytes(2, 13456) && prune_lds_bytes(1, 13456) == 89424 - 2 * 13456 && prune_lds_bytes(1, 13456) == 62512);
}

/* the request as it was written out by hand before the layout had one definition; it then held a kept flag per merge cell, which only the
 * backward kernel uses: the forward kernel's request is smaller by those words */
static size_t prune_lds_bytes_by_hand(int pairs, int max_cells, int max_merge) {
    const size_t cap = pairs ? (size_t) (((max_cells + 1) / 2 + 3) & ~3) : (size_t) ((max_cells + 3) & ~3);
    const size_t dwords = 4 * 128 + 128 + 4 * 128 + 64 + 2 * 1024 + 512 + 512 + 2 * 128 + 2 * 128 + 512 + 512 + 4 * 5 * 128 + 512;
    return dwords * 4 + (size_t) (((max_merge + 127) >> 7) << 2) * 4 + 2 * cap * 2 + 16;
}

/* The regions of the prune kernel's LDS (mrp_prune_lds.h): in order, without overlap, aligned as the kernel reads them, and the request
 * is their end plus the tail slack; the pointers handed out are the offsets. */
static void check_prune_lds_layout() {
    CHECK(PRUNE_SP == 128 && PRUNE_TAB == 5 && PRUNE_HIST == 1024 && PRUNE_SIDE == 128 && PRUNE_BMP == 512 && PRUNE_CHUNK == 512 && PRUNE_HTAB == 256 &&
          PRUNE_LDS_TAIL_SLACK == 16);
    CHECK(prune_flag_words(1) == 4 && prune_flag_words(128) == 4 && prune_flag_words(129) == 8 && prune_flag_words(13456) == 424);
    std::vector<uint32_t> block(prune_lds_bytes(0, MRP_PRUNE_MAX_CELLS) / 4);
    for (int pairs = 0; pairs < 3; pairs++)
        for (int cells = 1; cells <= MRP_PRUNE_MAX_CELLS; cells += 97) {
            const PruneLdsOff o = prune_lds_offsets(pairs != 0, cells);
            /* (dwords) every region with the size the kernel uses of it; the bins: two columns of 16-bit entries */
            const struct { int at, size, align; } R[] = {
                {o.sel, 4 * PRUNE_SP, 2}, {o.um, PRUNE_SP, 1}, {o.s1, 4 * PRUNE_SP, 2}, {o.sh, 64, 4}, {o.hist, 2 * PRUNE_HIST, 1}, {o.bmp_c, PRUNE_BMP, 1},
                {o.bmp_m, PRUNE_BMP, 1}, {o.kml, 2 * PRUNE_SP, 1}, {o.minfo, 2 * PRUNE_SP, 4}, {o.heads, PRUNE_CHUNK, 1}, {o.pref, PRUNE_BMP, 1},
                {o.tab, 2 * 2 * PRUNE_TAB * PRUNE_SIDE, 1}, {o.htab_key, PRUNE_HTAB, 1}, {o.htab_val, PRUNE_HTAB, 1}, {o.bins, o.cap_c, 4}};
            int at = 0;
            for (const auto &r : R) {
                CHECK(r.at == at && r.size > 0 && r.at % r.align == 0);
                at += r.size;
            }
            CHECK(o.end == at && (size_t) o.end * 4 + PRUNE_LDS_TAIL_SLACK == prune_lds_bytes(pairs, cells));
            CHECK((o.sh + MB_COL) % 4 == 0 && MB_COL + 8 <= MB_HIST_USED && MB_HIST_USED + 2 <= 64);
            CHECK(o.cap_c == prune_bins_cap(pairs != 0, cells) && o.cap_c % 4 == 0 && o.cap_c >= (pairs ? (cells + 1) / 2 : cells));
            for (int merge : {1, cells, MRP_PRUNE_MAX_CELLS})
                CHECK(prune_lds_bytes(pairs, cells) == prune_lds_bytes_by_hand(pairs, cells, merge) - 4 * (size_t) prune_flag_words(merge));
            const PruneLds l = prune_lds_carve(block.data(), pairs != 0, cells);
            CHECK(l.sel == block.data() + o.sel && l.um == block.data() + o.um && l.s1 == block.data() + o.s1 && l.sh == block.data() + o.sh);
            CHECK(l.hist == block.data() + o.hist && l.bmp_c == block.data() + o.bmp_c && l.bmp_m == block.data() + o.bmp_m && l.kml == block.data() + o.kml);
            CHECK(l.minfo == block.data() + o.minfo && l.heads == block.data() + o.heads && l.pref == block.data() + o.pref && l.tab == block.data() + o.tab);
            CHECK(l.htab_key == block.data() + o.htab_key && l.htab_val == block.data() + o.htab_val);
            CHECK(l.bins == reinterpret_cast<uint16_t *>(block.data() + o.bins) && l.cap_c == o.cap_c);
            CHECK((size_t) (reinterpret_cast<uint32_t *>(l.bins + 2 * l.cap_c) - block.data()) * 4 + PRUNE_LDS_TAIL_SLACK == prune_lds_bytes(pairs, cells));
        }
}

/* The cross product + emission plan, restated: a level that is mostly the single-wave kernel's runs the table-free mode 1 and, if any
 * column can exceed a wave (64 cells), mode 2 for the rest, with the narrow table; any other level runs mode 0, with the wide table
 * once a column can exceed two waves (128 cells). */
static void check_cross_emit_plan() {
    for (int32_t max_cells : {1, 63, 64, 65, 127, 128, 129, 256, 4096, 13456})
        for (int narrow = 0; narrow < 2; narrow++) {
            const CrossEmitPlan p = cross_emit_plan(max_cells, narrow != 0);
            if (narrow) {
                CHECK(!p.mode0 && p.mode1 && p.mode2 == (max_cells >= 65) && !p.wide_cap);
                CHECK(p.census_slot == (max_cells >= 65 ? CENSUS_XE_MODES_1_2 : CENSUS_XE_MODE1_ALONE));
            } else {
                CHECK(p.mode0 && !p.mode1 && !p.mode2 && p.wide_cap == (max_cells >= 129));
                CHECK(p.census_slot == (max_cells >= 129 ? CENSUS_XE_MODE0_WIDE_CAP : CENSUS_XE_MODE0_NARROW_CAP));
            }
        }
}

/* the census: every slot has a name, the names are distinct, there is none outside the table; the sweep classes have their slots */
static void check_census_slots() {
    for (int q = 0; q < CENSUS_SLOTS; q++) {
        CHECK(census_slot_name(q) != nullptr && census_slot_name(q)[0] != 0);
        for (int r = 0; r < q; r++) CHECK(strcmp(census_slot_name(q), census_slot_name(r)) != 0);
    }
    CHECK(census_slot_name(-1) == nullptr && census_slot_name(CENSUS_SLOTS) == nullptr);
    CHECK(strcmp(census_slot_name(census_prune_slot(PRUNE_1024, 1)), "prune_1024_pairs_over_cells") == 0);
    CHECK(strcmp(census_slot_name(census_prune_slot(PRUNE_512X10_TWO_GROUPS, 0)), "prune_512x10_two_groups_general") == 0);
    CHECK(strcmp(census_slot_name(census_prune_slot(PRUNE_256, 2)), "prune_256_units") == 0);
    CHECK(census_sweep_slot(sweep_class(256, 9000)) == CENSUS_SWEEP_NARROW && census_sweep_slot(sweep_class(257, 4096)) == CENSUS_SWEEP_MID &&
          census_sweep_slot(sweep_class(257, 4097)) == CENSUS_SWEEP_WIDE);
    LaunchCensus c;
    c.bump(CENSUS_MINI); c.bump(CENSUS_MINI); c.bump(CENSUS_SLOTS - 1);
    for (int q = 0; q < CENSUS_SLOTS; q++) CHECK(c.n[q].load() == (q == CENSUS_MINI ? 2u : q == CENSUS_SLOTS - 1 ? 1u : 0u));
}

struct Twenty { char b[20]; }; /* the size of a FragSite */

/* one pass over a count list, the element type chosen by position; returns the bytes used */
static size_t carve(void *block, const std::vector<size_t> &counts, std::vector<char *> &at, std::vector<size_t> &bytes) {
    BlockCarver c(block);
    at.clear(); bytes.clear();
    for (size_t k = 0; k < counts.size(); k++) {
        switch (k % 5) {
        case 0: at.push_back((char *) c.take<char>(counts[k])); bytes.push_back(counts[k]); break;
        case 1: at.push_back((char *) c.take<uint16_t>(counts[k])); bytes.push_back(2 * counts[k]); break;
        case 2: at.push_back((char *) c.take<int32_t>(counts[k])); bytes.push_back(4 * counts[k]); break;
        case 3: at.push_back((char *) c.take<double>(counts[k])); bytes.push_back(8 * counts[k]); break;
        default: at.push_back((char *) c.take<Twenty>(counts[k])); bytes.push_back(20 * counts[k]); break;
        }
    }
    return c.used;
}

static void check_carver(std::mt19937 &rng) {
    std::vector<size_t> counts(1 + rng() % 12);
    for (size_t &c : counts) c = rng() % 4 == 0 ? 0 : rng() % 3 == 0 ? 1 + rng() % 5000 : 1 + rng() % 70;
    std::vector<char *> at, at0;
    std::vector<size_t> bytes, bytes0;
    const size_t size = carve(nullptr, counts, at0, bytes0);
    for (char *p : at0) CHECK(p == nullptr);
    char *block = (char *) aligned_alloc(64, size + 64);
    CHECK(block != nullptr);
    CHECK(carve(block, counts, at, bytes) == size);
    size_t expect = 0;
    for (size_t k = 0; k < counts.size(); k++) {
        CHECK(((uintptr_t) at[k] & 63) == 0);
        CHECK(at[k] == block + expect); /* inside the block, behind every region before it */
        CHECK(at[k] + bytes[k] <= block + size);
        if (k + 1 < counts.size()) CHECK(at[k] + bytes[k] <= at[k + 1]);
        if (counts[k] == 0 && k + 1 < counts.size()) CHECK(at[k + 1] == at[k]); /* a zero count takes nothing */
        expect += (bytes[k] + 63) / 64 * 64;
        for (size_t q = 0; q < bytes[k]; q++) at[k][q] = (char) k; /* (the sanitizer watches the writes) */
    }
    CHECK(expect == size);
    free(block);
}

/* the chunk block of a work queue's batch (mrp_chunk_block_create): a few chunks carved one behind the other, sized first, then placed */
static void check_chunk_block(const std::vector<int> &n_sites, const std::vector<size_t> &pool_bytes, bool with_pool) {
    static const uint32_t ALLELES[] = {3, 2, 5, 1, 2}; /* slot totals 3, 5, 10, 11, 13: none divisible by 4 */
    const size_t n = n_sites.size();
    std::vector<size_t> alleles(n, 0), subs(n, 0), at(n + 1, 0);
    BlockCarver sizes(nullptr, MRP_CHUNK_BLOCK_ALIGN);
    for (size_t k = 0; k < n; k++) {
        for (int i = 0; i < n_sites[k]; i++) { alleles[k] += ALLELES[i]; subs[k] += ALLELES[i] * ALLELES[i]; }
        CHECK(n_sites[k] == 0 || alleles[k] % 4 != 0);
        const ChunkSlices z = carve_chunk(sizes, (size_t) n_sites[k], alleles[k], subs[k], pool_bytes[k], with_pool);
        CHECK(!z.allele_number && !z.allele_offset && !z.sub_offset && !z.same_until && !z.sub && !z.prior && !z.pool);
        at[k + 1] = sizes.used;
    }
    const size_t reserved = chunk_block_bytes(sizes.used);
    char *block = (char *) aligned_alloc(MRP_CHUNK_BLOCK_ALIGN, (reserved + MRP_CHUNK_BLOCK_ALIGN - 1) / MRP_CHUNK_BLOCK_ALIGN * MRP_CHUNK_BLOCK_ALIGN);
    CHECK(block != nullptr);
    char *end_before = block;
    for (size_t k = 0; k < n; k++) {
        BlockCarver c(block + at[k], MRP_CHUNK_BLOCK_ALIGN); /* as the second pass does: every chunk from its own offset */
        const ChunkSlices z = carve_chunk(c, (size_t) n_sites[k], alleles[k], subs[k], pool_bytes[k], with_pool);
        CHECK(at[k] + c.used == at[k + 1]); /* the sizing pass equals the pointer pass */
        const size_t ns = (size_t) n_sites[k];
        char *const p[7] = {(char *) z.allele_number, (char *) z.allele_offset, (char *) z.sub_offset, (char *) z.same_until, (char *) z.sub, (char *) z.prior, (char *) z.pool};
        const size_t bytes[7] = {4 * ns, 4 * (ns + 1), 4 * (ns + 1), 4 * ns, 2 * subs[k], 2 * alleles[k], pool_bytes[k]};
        CHECK((z.pool != nullptr) == with_pool);
        for (int q = 0; q < (with_pool ? 7 : 6); q++) {
            CHECK(((uintptr_t) p[q] & (MRP_CHUNK_BLOCK_ALIGN - 1)) == 0);
            CHECK(p[q] >= end_before && p[q] + bytes[q] <= block + sizes.used); /* inside the block, behind every slice before it */
            if (q > 0 && bytes[q - 1] == 0) CHECK(p[q] == p[q - 1]);             /* a zero-length slice takes nothing */
            CHECK(p[q] - end_before < MRP_CHUNK_BLOCK_ALIGN);                    /* nothing but the rounding between two slices */
            memset(p[q], (int) q, bytes[q]);                                     /* (the sanitizer watches the writes) */
            end_before = p[q] + bytes[q];
        }
        /* the packing kernel's reach behind a pool stays inside the allocation, behind the last pool of the block too */
        if (with_pool) CHECK((char *) z.pool + pool_bytes[k] + MRP_POOL_TAIL_PAD <= block + reserved);
    }
    free(block);
}

int main() {
    std::mt19937 rng(20240611);
    for (int64_t n : {0, 1, 2, 63, 4096, 4097, 6000})
        for (int mode = 0; mode < 4; mode++)
            for (int units = 0; units < 2; units++)
                for (int rep = 0; rep < (n <= 63 ? 20 : 2); rep++) check_level(random_level(rng, n, mode), units != 0);
    check_prune_selector();
    check_prune_lds();
    check_prune_lds_layout();
    check_cross_emit_plan();
    check_census_slots();
    for (int rep = 0; rep < 2000; rep++) check_carver(rng);
    for (int with_pool = 0; with_pool < 2; with_pool++)
        for (size_t last_pool : {0, 1, 255, 256, 257})
            for (int last_sites : {0, 1, 5}) {
                check_chunk_block({last_sites}, {last_pool}, with_pool != 0);
                check_chunk_block({5, 0, 1, last_sites}, {257, 0, 255, last_pool}, with_pool != 0);
                check_chunk_block({last_sites, 1, 5}, {last_pool, 256, 1}, with_pool != 0);
            }
    printf("level order ok\n");
    return 0;
}
