/*
 * mrp_prune_ctx.h -- what the roles of mrp_prune_kernel (mrp_engine_kernels.hip) share: the kernel's inputs, the workgroup context every
 * role function takes, the development clocks, and the two steps the chain on complement pairs (mrp_prune_chain_pairs.h) and the general
 * chain (mrp_prune_chain_general.h) have in common.  The roles: mrp_prune_lists.h (waves 1 and 2), mrp_prune_feed.h (wave 3, waves 4..).
 */
#ifndef MRP_PRUNE_CTX_H_
#define MRP_PRUNE_CTX_H_

#include "mrp_engine.h"
#include "mrp_prune_lds.h"
#include "mrp_wave.h"

struct PruneIn {
    const SweepCol *scols;
    const CrossCol *ccols;
    const int32_t *cell_f32, *cell_b32, *merge_f32, *merge_b32;
    const double *hmm_fb;
};

/* One workgroup at one hmm.  The arrays' structs and the hmm's record are the kernel's own (references: a copy of PruneScratch costs
 * SGPR spills in every instantiation); the parameters are a copy -- a dozen scalars, and with a reference the list stages keep more of
 * the kernel's arguments alive across their loops (two to five more spilled SGPRs in three instantiations).  errbits is the thread's,
 * reported by the kernel behind the roles.  A role function names what it uses of this at its head (the clock macros below name hi_,
 * lane and sc). */
template <int T_, int CPT_, int NGRP_, int VEC_, bool PAIRS_>
struct PruneCtx {
    static constexpr int T = T_, CPT = CPT_, NGRP = NGRP_, VEC = VEC_;
    static constexpr bool PAIRS = PAIRS_;
    static constexpr int W = T / WAVE;
    static constexpr int NBG = (W - 4) / NGRP;  /* waves per bin-streaming group; none (T = 256): columns of at most 64 CPT cells, whose
                                                 * bins the table wave writes beside its tables -- four waves per workgroup, four
                                                 * workgroups per CU where the register file allows two of eight waves */
    static constexpr int LG = NBG > 0 ? NBG * WAVE : WAVE; /* lanes per group */
    static_assert((W == 4 || W >= 6) && ((W - 4) % NGRP) == 0 && (NGRP == 1 || NGRP == 2) && (VEC == 1 || VEC == 4), "role layout");
    const PruneLds &lds;
    const PruneIn &d;
    const PruneScratch &sc;
    const PruneParams p;
    const PruneHmm &h;
    int K, S;      /* columns of the hmm; slots per column of the kept lists */
    int32_t total; /* max mode: the same integer for every column */
    int nb;        /* posterior bins */
    int wave, lane;
    int64_t hi_;
    bool units;    /* the level's f, b and merge arrays hold one entry per unit (MRP_XF_UNITS) */
    int &errbits;
};

/* buffer descriptor over [p, p + bytes): both made wave-uniform for the compiler (cdna_hip_programming.md T8 / T20) */
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t prune_rsrc(const void *p, int bytes) {
    const uint64_t a = (uint64_t) p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) a), hi = __builtin_amdgcn_readfirstlane((uint32_t) (a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *) (((uint64_t) hi << 32) | lo), 0, bytes, 0x00020000);
}

/* profiling aid: build with -DPRUNE_EXP_CLOCK (both mrp_engine.cpp and mrp_engine_kernels.hip) to sum, for the first hmm of a launch, the
 * shader cycles each role spends working and waiting at the column barrier (printed by mrp_engine.cpp under MRP_TIMING) */
#ifdef PRUNE_EXP_CLOCK
#define ROLE_CLK_INIT() uint64_t clk_work = 0, clk_wait = 0, clk_t = __builtin_amdgcn_s_memtime()
#define ROLE_BARRIER() do { const uint64_t t1_ = __builtin_amdgcn_s_memtime(); lds_barrier(); const uint64_t t2_ = __builtin_amdgcn_s_memtime(); \
                            clk_work += t1_ - clk_t; clk_wait += t2_ - t1_; clk_t = t2_; } while (0)
#define ROLE_CLK_DONE(slot) do { if (hi_ == 0 && lane == 0) { atomicAdd((unsigned long long *) (sc.err + 4) + 2 * (slot), (unsigned long long) clk_work); \
                                 atomicAdd((unsigned long long *) (sc.err + 4) + 2 * (slot) + 1, (unsigned long long) clk_wait); } } while (0)
#else
#define ROLE_CLK_INIT() do { } while (0)
#define ROLE_BARRIER() lds_barrier()
#define ROLE_CLK_DONE(slot) do { } while (0)
#endif

#ifdef PRUNE_EXP_CLOCK2 /* sections of the chain wave instead: kept merge cells, candidates, histogram + cutoff, selection, ties, next merge cells */
#define SEC_INIT() uint64_t sec_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; uint64_t sec_t = __builtin_amdgcn_s_memtime()
#define SEC_COUNT(i) do { sec_[i] += 1; } while (0) /* columns by path: 8 keep-all, 9 sorted, 10 histogram (one chunk), 11 histogram (several chunks) */
#define SEC(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); sec_[i] += t_ - sec_t; sec_t = t_; } while (0)
#define SEC_DONE() do { if (hi_ == 0 && lane == 0) for (int i_ = 0; i_ < 12; i_++) atomicAdd((unsigned long long *) (sc.err + 4) + i_, (unsigned long long) sec_[i_]); } while (0)
#else
#define SEC_INIT() do { } while (0)
#define SEC(i) do { } while (0)
#define SEC_COUNT(i) do { } while (0)
#define SEC_DONE() do { } while (0)
#endif

/* Cutoff bin and quota of a column whose candidates' posterior bins are counted in the histogram hk: lane l owns the 16 consecutive
 * bins [16 l, 16 l + 16); the histogram is stored lane-major, so these reads are conflict-free and the search has a fixed, short cost.
 * all: the column's candidates; kept_of(g): how many of them are kept when g pass the threshold.  n are kept: those of the bins
 * below B and the first `quota` of the in_B candidates of bin B (B = -1: none). */
struct PruneCutoff { int n, B, quota, in_B; };
template <class KeptOf>
static __device__ __forceinline__ PruneCutoff prune_cutoff(const uint32_t *hk, int lane, int thr_bin, bool thr_all, int all, KeptOf kept_of) {
    int v[16];
    int tot_l = 0, pass = 0;
    const int thr_rel = thr_bin - lane * 16; /* bins q <= thr_rel of this lane pass the threshold */
#pragma unroll
    for (int q = 0; q < 16; q++) {
        v[q] = (int) hk[q * WAVE + lane];
        tot_l += v[q];
        if (q <= thr_rel) pass += v[q];
    }
    const int incl = wave_incl_scan(tot_l, lane);
    const int g = thr_all ? all : __builtin_amdgcn_readlane(wave_incl_scan(pass, lane), WAVE - 1);
    const int n = kept_of(g);
    const int ex = incl - tot_l;
    int myq = -1, myQ = 0, myV = 0;
    const bool owner_lane = n > 0 && ex < n && n <= incl;
    if (owner_lane) {
        int cum = ex;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            if (myq < 0 && cum + v[q] >= n) { myq = q; myQ = n - cum; myV = v[q]; }
            cum += v[q];
        }
    }
    const int myB = lane * 16 + myq;
    const uint64_t om = __ballot(owner_lane);
    const int srcu = __builtin_amdgcn_readfirstlane(om ? __ffsll((unsigned long long) om) - 1 : 0);
    PruneCutoff c;
    c.n = n;
    c.B = om ? __builtin_amdgcn_readlane(myB, srcu) : -1;
    c.quota = om ? __builtin_amdgcn_readlane(myQ, srcu) : 0;
    c.in_B = om ? __builtin_amdgcn_readlane(myV, srcu) : 0;
    return c;
}

/* The candidates of the cutoff bin are marked in the bitmap bmp_c by cell (unit) index; a candidate's rank in list order is the number
 * of marks below it -- marks before its bitmap word (pref: prefix counts, lane l owns words 8 l .. 8 l + 7) plus those below it in
 * the word.  Fenced on both sides. */
static __device__ __forceinline__ void prune_bitmap_prefix(const uint32_t *bmp_c, uint32_t *pref, int lane) {
    wave_lds_fence();
    {
        uint32_t w[8];
        int cnt_l = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) { w[q] = bmp_c[lane * 8 + q]; cnt_l += __popc(w[q]); }
        int run = wave_incl_scan(cnt_l, lane) - cnt_l;
#pragma unroll
        for (int q = 0; q < 8; q++) { pref[lane * 8 + q] = (uint32_t) run; run += __popc(w[q]); }
    }
    wave_lds_fence();
}

#endif
