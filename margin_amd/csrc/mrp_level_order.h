/*
 * mrp_level_order.h -- what staging a resident level (mrp_engine.cpp) decides by host arithmetic alone: the order of the level's
 * hmms, their launch classes (the recursion's, the prune kernel's, the cross product + emission plan) and their census slots, and the
 * layout of its page-locked blocks; also the layout of a work queue's chunk block
 * (mrp_chunk.cpp).  No HIP call: tests/level_order_check.cpp runs it on the CPU.
 */
#ifndef MRP_LEVEL_ORDER_H_
#define MRP_LEVEL_ORDER_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "mrp_census.h"
#include "mrp_engine.h" /* MRP_MINI_MAX_UNITS, MRP_PRUNE_MAX_CELLS */
#include "mrp_prune_lds.h"
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

/* The instantiation of the prune kernel for a level (mrp_launch_prune), by what its bin-streaming waves hold per column -- cells, or
 * units where the level's arrays hold units (pairs == 2) -- in registers:
 *   up to   256  four waves, the table wave writes the bins (the first merge levels: a few reads per hmm)
 *   up to 4 096  two groups of 2 waves x 32 entries per lane
 *   up to 5 120  two groups of 2 waves x 10 16-byte loads per lane, alternating over the columns
 *   up to 10 240 one group of 4 waves x 10 16-byte loads per lane
 *   beyond       1 024 threads: two groups of 6 waves x 36 entries; a level of more than MRP_PRUNE_MAX_CELLS cells is refused */
#define MRP_PRUNE_HELD_256 (4 * 64)
#define MRP_PRUNE_HELD_512X32 (2 * 64 * 32)
#define MRP_PRUNE_HELD_TWO_GROUPS (2 * 64 * 10 * 4)
#define MRP_PRUNE_HELD_ONE_GROUP (4 * 64 * 10 * 4)
static inline int prune_held(int pairs, int max_cells) { return pairs == 2 ? (max_cells + 1) / 2 : max_cells; }
static inline PruneClass prune_class(int pairs, int max_cells) {
    if (max_cells > MRP_PRUNE_MAX_CELLS) return PRUNE_TOO_LARGE;
    const int held = prune_held(pairs, max_cells);
    return held <= MRP_PRUNE_HELD_256 ? PRUNE_256 : held <= MRP_PRUNE_HELD_512X32 ? PRUNE_512X32 :
           held <= MRP_PRUNE_HELD_TWO_GROUPS ? PRUNE_512X10_TWO_GROUPS : held <= MRP_PRUNE_HELD_ONE_GROUP ? PRUNE_512X10_ONE_GROUP : PRUNE_1024;
}
/* The prune kernel's dynamic LDS, the same for every class: prune_lds_bytes and the layout it is the size of, mrp_prune_lds.h (PRUNE_SP,
 * PRUNE_TAB).  The largest request of the path is the per-cell level of 116 x 116 cells under the general chain: 89 424 bytes, within
 * MRP_LDS_BUDGET (tests/level_order_check.cpp), so no reachable level is refused for its LDS. */

static inline int census_prune_slot(PruneClass k, int pairs) { return CENSUS_PRUNE + (int) k * PRUNE_CHAIN_MODES + pairs; }

/* What mrp_launch_cross_emit launches for a level: the modes of the one-pass cross product + emission kernel and the table dwords
 * per wave.  level_max_cells: the level's largest column by the static bounds; up to 128 cells (64 array entries of a unit level)
 * every column has a lane per entry.  mostly_narrow: most hmms of the level are the single-wave kernel's -- mode 1 takes the
 * table-free columns, mode 2 the rest (a column of at most 64 cells is narrow whatever its parents: they have no more cells than
 * it has, so mode 1 runs alone). */
struct CrossEmitPlan {
    bool mode0, mode1, mode2;
    bool wide_cap; /* XE_CAP_WIDE, not XE_CAP_NARROW */
    int census_slot;
};
static inline CrossEmitPlan cross_emit_plan(int32_t level_max_cells, bool mostly_narrow) {
    CrossEmitPlan p{};
    p.wide_cap = level_max_cells > 2 * 64 && !mostly_narrow;
    p.mode0 = !mostly_narrow;
    p.mode1 = mostly_narrow;
    p.mode2 = mostly_narrow && level_max_cells > 64;
    p.census_slot = p.mode0 ? (p.wide_cap ? CENSUS_XE_MODE0_WIDE_CAP : CENSUS_XE_MODE0_NARROW_CAP) : p.mode2 ? CENSUS_XE_MODES_1_2 : CENSUS_XE_MODE1_ALONE;
    return p;
}

static inline int census_sweep_slot(SweepClass k) { return k == SWEEP_NARROW ? CENSUS_SWEEP_NARROW : k == SWEEP_MID ? CENSUS_SWEEP_MID : CENSUS_SWEEP_WIDE; }

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
