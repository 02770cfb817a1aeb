/*
 * mrp_level_order.h -- what staging a resident level (mrp_engine.cpp) decides by host arithmetic alone: the order of the level's
 * hmms, their launch classes, and the layout of its page-locked blocks; also the layout of a work queue's chunk block
 * (mrp_chunk.cpp).  No HIP call: tests/level_order_check.cpp runs it on the CPU.
 */
#ifndef MRP_LEVEL_ORDER_H_
#define MRP_LEVEL_ORDER_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "mrp_engine.h" /* MRP_MINI_MAX_UNITS */
#include "rphmm_host.h" /* mrp_xhmm */

/* Hands out consecutive aligned regions of one block (64 bytes unless told otherwise; a power of two).  Run the same code twice:
 * without a base, `used` is the size to reserve; with the block's address, take() returns the regions. */
struct BlockCarver {
    char *base;
    size_t align, used = 0;
    explicit BlockCarver(void *block = nullptr, size_t alignment = 64) : base(static_cast<char *>(block)), align(alignment) {}
    template <class T> T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += (count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
};

/* One chunk's share of the block that holds the chunks of a work queue's batch: the six site tables, then the profile bytes
 * unless they are on the device already (with_pool = false: pool stays NULL and takes nothing).  Every slice starts on a
 * multiple of MRP_CHUNK_BLOCK_ALIGN bytes.  The block is reserved MRP_CHUNK_BLOCK_SLACK bytes larger than the slices need, which
 * covers the packing kernel's reach behind the last chunk's profile bytes (MRP_POOL_TAIL_PAD, mrp_kernels.h). */
#define MRP_CHUNK_BLOCK_ALIGN 256
#define MRP_CHUNK_BLOCK_SLACK 256
static_assert(MRP_CHUNK_BLOCK_SLACK >= MRP_POOL_TAIL_PAD, "the chunk block ends too close behind its last profile pool");
static inline size_t chunk_block_bytes(size_t carved) { return carved + MRP_CHUNK_BLOCK_SLACK; }
struct ChunkSlices { uint32_t *allele_number, *allele_offset, *sub_offset; int32_t *same_until; uint16_t *sub, *prior; uint8_t *pool; };
static inline ChunkSlices carve_chunk(BlockCarver &c, size_t n_sites, size_t n_alleles, size_t n_sub, size_t pool_bytes, bool with_pool) {
    ChunkSlices s{};
    s.allele_number = c.take<uint32_t>(n_sites); s.allele_offset = c.take<uint32_t>(n_sites + 1); s.sub_offset = c.take<uint32_t>(n_sites + 1);
    s.same_until = c.take<int32_t>(n_sites); s.sub = c.take<uint16_t>(n_sub); s.prior = c.take<uint16_t>(n_alleles);
    if (with_pool) s.pool = c.take<uint8_t>(pool_bytes);
    return s;
}

struct LevelClass {
    std::vector<int32_t> order; /* indices into x */
    int max_merge = 1;          /* largest bound_max_merge of the class; on unit levels halved + 1 (one entry per pair: half the LDS) */
};

/* kept with the level object: the arrays keep their capacity from level to level */
struct LevelOrder {
    std::vector<int32_t> perm, pos; /* position in the level's PruneHmm array -> index into x, and its inverse */
    int64_t n_mini = 0;             /* hmms of the single-wave kernel: the last n_mini positions */
    LevelClass wide, mid, narrow;   /* launch classes of the recursion kernel (the single-wave hmms are in none) */
    int32_t max_cells = 1, max_merge = 1;     /* largest bound_max_cells / bound_max_merge of the level */
    int64_t bound_cells = 0, bound_merge = 0; /* sums of the hmms' static bounds (cells padded to a multiple of 4 per hmm) */
    std::vector<int64_t> at;                           /* scratch of level_sort */
    std::vector<std::pair<int64_t, int32_t>> keys;     /* scratch of level_classes */
};

/* hmms whose columns hold at most 64 units and 64 merge units (the static bounds count cells) go through recursion, prune
 * and compaction on ONE wave each (mrp_mini_kernel): the first merge levels, tens of thousands of hmms of a few cells.
 * They sit at the end of the level's PruneHmm array; unit levels only. */
static inline bool level_is_mini(const mrp_xhmm &h, bool units) {
    return units && h.bound_max_cells <= 2 * MRP_MINI_MAX_UNITS && h.bound_max_merge <= 2 * MRP_MINI_MAX_UNITS;
}

/* perm, pos, n_mini.  The prune kernel walks one hmm per workgroup, its columns one after the other: longest hmms first.
 * Stable counting sort by descending number of columns, the single-wave class behind the others. */
static inline void level_sort(const mrp_xhmm *x, int64_t n, bool units, LevelOrder &o) {
    o.perm.resize((size_t) n);
    o.pos.resize((size_t) n);
    o.n_mini = 0;
    int32_t max_cols = 1;
    for (int64_t i = 0; i < n; i++) max_cols = std::max(max_cols, x[i].n_cols);
    const size_t half = (size_t) max_cols + 1;
    o.at.assign(2 * half + 1, 0);
    auto slot_of = [&](int64_t i) { return (size_t) (max_cols - x[i].n_cols) + (level_is_mini(x[i], units) ? half : 0); };
    for (int64_t i = 0; i < n; i++) { o.at[slot_of(i) + 1]++; if (level_is_mini(x[i], units)) o.n_mini++; }
    for (size_t q = 1; q < o.at.size(); q++) o.at[q] += o.at[q - 1];
    for (int64_t i = 0; i < n; i++) o.perm[(size_t) o.at[slot_of(i)]++] = (int32_t) i;
    for (int64_t j = 0; j < n; j++) o.pos[(size_t) o.perm[(size_t) j]] = (int32_t) j;
}

/* The launch class of the recursion kernel for an hmm, by its largest column and largest merge column: the rule of the resident
 * levels (level_classes, from the static bounds) and of the host-fed batch's int32 plan (mrp_batch_upload). */
enum SweepClass { SWEEP_NARROW, SWEEP_MID, SWEEP_WIDE };
static inline SweepClass sweep_class(int64_t max_cells, int64_t max_merge) {
    return max_cells <= 256 ? SWEEP_NARROW : max_merge <= 4096 ? SWEEP_MID : SWEEP_WIDE;
}

/* the launch classes, from the static bounds; largest first inside a class.  Also the level's maxima and bound sums. */
static inline void level_classes(const mrp_xhmm *x, int64_t n, bool units, LevelOrder &o) {
    o.wide.order.clear(); o.mid.order.clear(); o.narrow.order.clear();
    o.max_cells = o.max_merge = 1;
    o.bound_cells = o.bound_merge = 0;
    for (int64_t i = 0; i < n; i++) {
        const mrp_xhmm &q = x[i];
        o.max_cells = std::max(o.max_cells, q.bound_max_cells);
        o.max_merge = std::max(o.max_merge, q.bound_max_merge);
        o.bound_cells += (q.bound_cells + 3) & ~3ll;
        o.bound_merge += q.bound_merge;
        if (level_is_mini(q, units)) continue; /* swept by the single-wave kernel */
        const SweepClass k = sweep_class(q.bound_max_cells, q.bound_max_merge);
        LevelClass &c = k == SWEEP_NARROW ? o.narrow : k == SWEEP_MID ? o.mid : o.wide;
        c.order.push_back((int32_t) i);
    }
    for (LevelClass *c : {&o.wide, &o.mid, &o.narrow}) {
        /* largest first, so that the long chains start early; a class of many thousand hmms (the first merge levels: a few
         * cells each, a level of 25 000) has no tail worth 1.5 ms of sorting on the thread that feeds the device */
        if (c->order.size() <= 4096) {
            o.keys.clear();
            for (int32_t i : c->order) o.keys.push_back({-x[i].bound_cells, i});
            std::sort(o.keys.begin(), o.keys.end());
            for (size_t j = 0; j < o.keys.size(); j++) c->order[j] = o.keys[j].second;
        }
        int m = 1;
        for (int32_t i : c->order) m = std::max(m, x[i].bound_max_merge);
        /* the merge columns of a unit level hold one entry per pair (the bounds count cells): half the LDS per workgroup */
        c->max_merge = units ? (m + 1) / 2 + 1 : m;
    }
}

#endif
