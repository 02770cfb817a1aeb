/*
 * level_order_check.cpp -- the host arithmetic of staging a resident level (margin_amd/csrc/mrp_level_order.h) without a device:
 * the order and launch classes of random levels against a plain restatement, the block carver's two passes against each other, and
 * the layout of a work queue's chunk block.
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
