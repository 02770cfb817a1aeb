/*
 * mrp_census.h -- the launch census of the device-resident path: one counter per launch class, kept on the context and bumped by
 * the launchers whenever a class is launched with work.  It says WHICH of the size-class kernels a call ran (every class is its own
 * register blocking, barrier pattern and LDS layout), which no result can say.  Read by mrp_context_launch_census
 * (include/margin_rphmm.h: test suite and probes only).  No HIP call: tests/level_order_check.cpp checks the slot arithmetic.
 */
#ifndef MRP_CENSUS_H_
#define MRP_CENSUS_H_

#include <atomic>
#include <cstdint>

/* the five instantiations of mrp_prune_kernel<T, CPT, NGRP, VEC, PAIRS> by what the bin-streaming waves hold (prune_class) ... */
enum PruneClass { PRUNE_256, PRUNE_512X32, PRUNE_512X10_TWO_GROUPS, PRUNE_512X10_ONE_GROUP, PRUNE_1024, PRUNE_CLASSES, PRUNE_TOO_LARGE = -1 };
/* ... times the chain mode, PruneParams.pairs: 0 general, 1 complement pairs over per-cell arrays, 2 units */
enum { PRUNE_CHAIN_MODES = 3 };

enum CensusSlot {
    CENSUS_PRUNE = 0, /* + PruneClass * PRUNE_CHAIN_MODES + PruneParams.pairs */
    CENSUS_PRUNE_BACK_GENERAL = CENSUS_PRUNE + PRUNE_CLASSES * PRUNE_CHAIN_MODES,
    CENSUS_PRUNE_BACK_PAIRS,
    CENSUS_XE_MODE0_NARROW_CAP, /* cross product + emission in one pass (mrp_launch_cross_emit, cross_emit_plan) */
    CENSUS_XE_MODE0_WIDE_CAP,
    CENSUS_XE_MODE1_ALONE,
    CENSUS_XE_MODES_1_2,
    CENSUS_CROSS_TWO_KERNELS,   /* mrp_launch_cross: the final level, the ancestor model, test hook bit 1 */
    CENSUS_SWEEP_NARROW,        /* the recursion kernel's classes on resident levels (sweep_class) */
    CENSUS_SWEEP_MID,
    CENSUS_SWEEP_WIDE,
    CENSUS_MINI,                /* the single-wave kernel */
    CENSUS_COMPACT,
    CENSUS_TRACEBACK,
    CENSUS_FRAGMENTS,
    CENSUS_SLOTS
};

static inline const char *census_slot_name(int slot) {
    static const char *const NAMES[CENSUS_SLOTS] = {
        "prune_256_general", "prune_256_pairs_over_cells", "prune_256_units",
        "prune_512x32_general", "prune_512x32_pairs_over_cells", "prune_512x32_units",
        "prune_512x10_two_groups_general", "prune_512x10_two_groups_pairs_over_cells", "prune_512x10_two_groups_units",
        "prune_512x10_one_group_general", "prune_512x10_one_group_pairs_over_cells", "prune_512x10_one_group_units",
        "prune_1024_general", "prune_1024_pairs_over_cells", "prune_1024_units",
        "prune_back_general", "prune_back_pairs",
        "cross_emit_mode0_narrow_cap", "cross_emit_mode0_wide_cap", "cross_emit_mode1_alone", "cross_emit_modes_1_2",
        "cross_two_kernels",
        "sweep_narrow", "sweep_mid", "sweep_wide",
        "mini",
        "compact", "traceback", "fragments",
    };
    return slot >= 0 && slot < CENSUS_SLOTS ? NAMES[slot] : nullptr;
}

/* relaxed host atomics: the concurrent halves of a call launch from several host threads, and nothing is ordered by a count */
struct LaunchCensus {
    std::atomic<uint64_t> n[CENSUS_SLOTS];
    LaunchCensus() { for (auto &c : n) c.store(0, std::memory_order_relaxed); }
    void bump(int slot) { n[slot].fetch_add(1, std::memory_order_relaxed); }
};

#endif
