/*
 * mrp_engine.cpp -- host side of the device-resident merge level.
 *
 * One level performs, for a set of independent overlap components (coordination.c:285-328), what the reference does
 * with
 *     stRPHmm_createCrossProductOfTwoAlignedHmm (hmm.c:534)  ->  mrp_cross_kernel
 *     stRPHmm_forwardBackward (hmm.c:931)                    ->  packing / emission / recursion kernels
 *     stRPHmm_prune (hmm.c:1160)                             ->  mrp_prune_kernel + mrp_compact_kernel
 * without the hmm leaving HBM: the parents are read from, and the pruned result is written to, the fixed-stride
 * resident layout of mrp_engine.h.
 *
 * What the host contributes to a level does not depend on any result of the level before: the column structure of the
 * cross products (sites, reads, connector kinds) and the ADDRESSES at which the parents' per-column counts will be
 * found.  A level therefore goes through three steps:
 *     stage   host only: the static description (PlanCol / PlanHmm, read offsets, launch classes from static bounds) is
 *             built by the worker pool and uploaded on the copy stream -- while the level before is still running;
 *     launch  the layout kernels turn the parents' counts into sizes, offsets and every kernel descriptor; four totals
 *             come back (the only host wait of a level, it also ends the level before), the cell arrays are allocated
 *             and the level's kernels queued;
 *     end     per-hmm error flags (and, at the final level, the traced-back path) are read.
 * The structural decisions (tiling paths, overlap components, column alignment) are made by rphmm_host.c from read
 * intervals alone.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <new>
#include <vector>

#include "mrp_engine.h"
extern "C" void mrp_pool_set_tag(int t);
extern "C" void mrp_pool_set_weight(int ns_per_index);
#include "mrp_internal.h"
#include "mrp_level_order.h"

#define ENG_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace {
struct Segment { /* the pruned hmms produced by one level, and their column structure (read by the levels above) */
    DevBufGroup arrays;
    DevBuf<uint64_t> part{arrays};
    DevBuf<uint32_t> np{arrays};
    DevBuf<int32_t> n_cells{arrays}, n_merge{arrays};
    DevBuf<ResCol> cols{arrays};
    DevBuf<int64_t> rbo{arrays};
};

/* per hmm: where its columns, reads, allele slots and parents start in the level; the chunk table index; totals */
struct HmmIndex {
    std::vector<int64_t> col0, read0, slot0, par0, cost;
    std::vector<int32_t> chunk;
    int64_t total_cols = 0, total_reads = 0, total_slots = 0, total_par = 0;
};

/* the page-locked block holding every array of the static description that is uploaded */
struct StageBlock {
    XDesc *xd; mrp_xpar *par; int32_t *cstart, *croff; PlanHmm *phmm; PruneHmm *ph; int32_t *ord_w, *ord_m, *ord_n; DevChunk *chunks; SegDev *seg;
    size_t bytes;
    StageBlock() = default;
    StageBlock(void *block, size_t n, const HmmIndex &ix, size_t n_chunks) {
        BlockCarver c(block);
        xd = c.take<XDesc>(n); par = c.take<mrp_xpar>((size_t) ix.total_par);
        cstart = c.take<int32_t>((size_t) ix.total_cols + 1); croff = c.take<int32_t>((size_t) ix.total_cols);
        phmm = c.take<PlanHmm>(n); ph = c.take<PruneHmm>(n);
        ord_w = c.take<int32_t>(n); ord_m = c.take<int32_t>(n); ord_n = c.take<int32_t>(n);
        chunks = c.take<DevChunk>(n_chunks); seg = c.take<SegDev>(1);
        bytes = c.used;
    }
};

/* the second page-locked block: totals, error flags, final level: path and totals of the sweep */
struct ResultsBlock {
    int64_t *totals = nullptr;
    int32_t *err = nullptr, *err_hmm = nullptr, *path_cell = nullptr;
    uint64_t *path_part = nullptr;
    double *fb = nullptr;
    size_t bytes = 0;
    ResultsBlock() = default;
    ResultsBlock(void *block, size_t n, size_t total_cols, bool final_level) {
        BlockCarver c(block);
        totals = c.take<int64_t>(8); err = c.take<int32_t>(16); err_hmm = c.take<int32_t>(n);
        if (final_level) { path_part = c.take<uint64_t>(total_cols); fb = c.take<double>(2 * n); path_cell = c.take<int32_t>(total_cols); }
        bytes = c.used;
    }
};

/* genome fragments of a final level on the device (mrp_fragment_kernel): inputs staged, results fetched with the level's */
struct FragStage {
    bool on = false;
    DevBufGroup arrays;
    DevBuf<FragHmm> d_hmms{arrays};
    DevBuf<FragRead> d_reads{arrays};
    DevBuf<int32_t> d_by_pool{arrays}, d_disc{arrays}, d_lists{arrays}, d_work{arrays}, d_counts{arrays}, d_col_read{arrays}, d_col_cnt{arrays};
    DevBuf<FragSite> d_sites{arrays};
    DevBuf<uint64_t> d_col_part{arrays};
    DevBuf<uint32_t> d_read_key{arrays};
    PinnedBuf stage_block, results;
    std::vector<FragHmm> hmms; /* in the order of the level's PruneHmm array: the kernel indexes both alike */
    int64_t sites_total = 0, list_total = 0;
    FragSite *h_sites = nullptr; int32_t *h_lists = nullptr, *h_counts = nullptr;

    int stage(const mrp_xhmm *x, int64_t n, const std::vector<int32_t> &perm, const HmmIndex &ix, DevPool *pl, hipStream_t cs);
    FragArrays device_arrays() const {
        FragArrays fa{};
        fa.hmms = d_hmms.p; fa.reads = d_reads.p; fa.by_pool = d_by_pool.p; fa.discarded = d_disc.p;
        fa.sites = d_sites.p; fa.lists = d_lists.p; fa.work = d_work.p; fa.counts = d_counts.p;
        fa.col_read = d_col_read.p; fa.col_part = d_col_part.p; fa.read_key = d_read_key.p; fa.col_cnt = d_col_cnt.p;
        return fa;
    }
    int fetch(int64_t n, hipStream_t s);
    void scatter(mrp_xhmm *x, int64_t n, const std::vector<int32_t> &perm, const int32_t *err_hmm) const;
    void reset() { arrays.release(); on = false; }
};
}  // namespace

/* everything one level keeps between its staging and its completion */
struct mrp_engine_level_state {
    mrp_batch *b = nullptr;
    std::unique_ptr<Segment> seg;
    int seg_id = -1;
    mrp_xhmm *x = nullptr;
    int64_t n = 0;
    bool final_level = false;
    bool fused = false; /* cross product and emission in one kernel, no partition array (merge levels, no ancestor model) */
    bool units = false; /* the level's cell / merge cell arrays hold one entry per complement pair (MRP_XF_UNITS) */
    bool any_pack = true, any_planes = true; /* columns for the byte packing kernel / the bit plane kernel */
    bool deferred = false; /* launched without waiting for its totals: arrays sized by the static bounds (level_defers) */
    HmmIndex ix;
    LevelOrder order;
    PruneParams pp{};
    DevBufGroup arrays; /* every device array of the level but the segment's and the fragments' */
    /* static description, device side */
    DevBuf<PlanCol> d_plan{arrays};
    DevBuf<XDesc> d_xd{arrays};
    DevBuf<mrp_xpar> d_par{arrays};
    DevBuf<int32_t> d_cstart{arrays}, d_croff{arrays};
    DevBuf<PlanHmm> d_phmm{arrays};
    DevBuf<uint16_t> d_dims{arrays};
    DevBuf<LayoutTot> d_tot{arrays};
    DevBuf<LayoutBase> d_base{arrays};
    DevBuf<int64_t> d_totals{arrays}, d_tile_sums{arrays};
    /* what the layout kernels, the cross product and the prune write */
    DevBuf<CrossCol> d_cc{arrays};
    DevBuf<PruneHmm> d_ph{arrays};
    DevBuf<int32_t> d_col_hmm{arrays}, d_nkept{arrays}, d_nkeptm{arrays}, d_err{arrays}, d_err_hmm{arrays};
    DevBuf<uint16_t> d_kept{arrays}, d_keptm{arrays};
    DevBuf<uint32_t> d_kept_np{arrays};
    FragStage frag;
    PinnedBuf stage, results; /* host side of the uploads; of the results */
    StageBlock h;             /* pointers into them */
    ResultsBlock res;
    struct Timing { double begin = 0, staged = 0, launch_ms = 0, react_ms = 0, launched = 0; } t; /* react_ms: from the totals' arrival to the last kernel queued */
    unsigned long long clk[12] = {0};
    hipEvent_t lay0 = nullptr;     /* in front of the layout kernels (timing) */
    hipEvent_t uploaded = nullptr; /* end of the uploads on the copy stream */
    hipEvent_t done = nullptr;     /* behind everything the level queued on the main stream (its results' copies included) */
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; /* before / after the cross product, after the sweeps, after the compaction, [4] after the prune */
    hipError_t create_events() { /* once, when the level object is made */
        hipError_t he = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (he == hipSuccess) he = hipEventCreate(&lay0);
        if (he == hipSuccess) he = hipEventCreateWithFlags(&uploaded, hipEventDisableTiming);
        for (auto &e_ : ev)
            if (he == hipSuccess) he = hipEventCreate(&e_);
        return he;
    }
    /* back to the empty state: no device array, no hmms; the batch object goes back to the engine first (level_retire), the
     * page-locked blocks, the events and the host arrays' capacity stay for the next level */
    void reset() {
        seg.reset();
        arrays.release();
        frag.reset();
        order.perm.clear();
        x = nullptr; n = 0;
        deferred = false;
        t = Timing{};
    }
    ~mrp_engine_level_state() {
        for (hipEvent_t e_ : {uploaded, done, lay0, ev[0], ev[1], ev[2], ev[3], ev[4]})
            if (e_) (void) hipEventDestroy(e_);
        if (b) mrp_batch_destroy(b);
    }
};

struct mrp_engine {
    mrp_context *ctx = nullptr;
    mrp_params params{};
    PruneParams pp{};
    DevBufGroup arrays;
    DevBuf<uint64_t> leaf_part{arrays};
    DevBuf<uint32_t> leaf_np{arrays};
    DevBuf<int32_t> leaf_count{arrays};
    std::vector<std::unique_ptr<Segment>> segments;
    /* every staged level gets a segment number; its arrays are listed here (host copy + device table) for the levels above */
    static constexpr int MAX_SEGS = 64;
    SegDev segtab[MAX_SEGS] = {};
    int n_segs = 0;
    DevBuf<SegDev> d_segs{arrays};
    mrp_engine_stats stats{};
    mrp_engine_level_state *staged = nullptr;  /* staged, not launched */
    /* launched, not ended, oldest first.  A level is normally ended by the launch of the next one (the one host wait of a level: the
     * exact sizes of the next level's arrays come back with it).  Small levels -- a call of a few chunks, the first merge levels --
     * are launched WITHOUT that wait (deferred: arrays sized by the static bounds) and several of them are in flight at a time;
     * they are ended, in order, as their events complete. */
    std::vector<mrp_engine_level_state *> inflight;
    double diag_layout_gap_ms = 0, diag_react_ms = 0;
    std::vector<std::pair<long long, double>> timeline; /* MRP_TIMELINE: (hmms of the level, host time of its launch) */
    double t_created = 0;
    int64_t n_ended = 0;         /* levels ended so far (mrp_engine_levels_ended: the caller settles what it keeps per level) */
    int64_t inflight_bytes = 0;  /* device bytes of the deferred levels in flight (by their bounds) */
    std::vector<mrp_batch *> spare;            /* emptied batch objects (host arrays keep their capacity) */
    std::vector<mrp_engine_level_state *> spare_levels; /* level states whose pinned buffers are reused */
};

static double eng_now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * ts.tv_sec + 1e-6 * ts.tv_nsec;
}

/* device bytes of a level's cell arrays by its hmms' static bounds */
static int64_t level_bound_bytes(const mrp_engine_level_state *L) { return 16 * L->order.bound_cells + 8 * L->order.bound_merge; }

/* back to the empty state; the batch object and the pinned buffers stay with the engine for the next level */
static void level_retire(mrp_engine *e, mrp_engine_level_state *L, bool complete = false) {
    if (!L) return;
    mrp_context *ctx = e->ctx;
    (void) hipSetDevice(ctx->device);
    if (!complete) { /* (complete: the level's `done` event has been seen -- everything that touches its buffers is over, while later
                      *  levels may still be queued on the stream) */
        (void) ctx->wait_stream(ctx->stream); /* before the buffers go back to the pool */
        if (ctx->pre) (void) ctx->wait_stream(ctx->pre);
    }
    if (L->b) {
        L->b->recycle();
        e->spare.push_back(L->b);
        L->b = nullptr;
    }
    if (L->deferred) e->inflight_bytes -= level_bound_bytes(L);
    L->reset();
    e->spare_levels.push_back(L);
    ctx->pool.reclaim(); /* the one place a level's arrays are released: the rule is stated at DevPool::reclaim() */
}

extern "C" {

int mrp_engine_create(mrp_context *ctx, const mrp_params *params, mrp_engine **out) {
    if (!ctx || !params || !out) return mrp_set_error(MRP_ERR_ARG, "mrp_engine_create: NULL argument");
    *out = nullptr;
    if (params->reserved != 0) return mrp_set_error(MRP_ERR_ARG, "mrp_params.reserved must be 0");
    if (!params->max_not_sum_transitions)
        return mrp_set_error(MRP_ERR_UNSUPPORTED, "the device-resident merge needs maxNotSumTransitions (integer posteriors)");
    const int64_t lim = std::max<int64_t>(params->min_partitions_in_a_column, params->max_partitions_in_a_column);
    if (lim < 1 || lim > MRP_PRUNE_MAX_S || params->min_partitions_in_a_column < 0)
        return mrp_set_error(MRP_ERR_UNSUPPORTED, "the device-resident merge keeps at most %d partitions per column", MRP_PRUNE_MAX_S);
    ENG_TRY(hipSetDevice(ctx->device));
    mrp_engine *e = new (std::nothrow) mrp_engine();
    if (!e) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    e->ctx = ctx;
    e->params = *params;
    e->t_created = eng_now();
    PruneParams &pp = e->pp;
    pp.S = (int32_t) ((lim + 3) & ~3ll);
    pp.min_p = (int32_t) params->min_partitions_in_a_column;
    pp.max_p = (int32_t) std::min<int64_t>(params->max_partitions_in_a_column, 1 << 20);
    if (pp.max_p < 0) pp.max_p = 0;
    /* the prune chain on complement pairs (mrp_prune_kernel<..., PAIRS>): every cell has its twin and the limits never cut
     * a pair.  Test hook bit 3 keeps the general chain for A/B parity. */
    pp.pairs = params->include_inverted_partitions && (pp.min_p & 1) == 0 && (pp.max_p & 1) == 0 ? 1 : 0;
    /* posterior = min(1, exp(s)), s = f + b - total an integer <= 0 (column.c:177-193).  Ranking by the
     * integer is ranking by the double as long as consecutive integers give distinct doubles; from the
     * underflow point of exp down every posterior is 0.0 and they all tie: that is the last bin. */
    int zero_bin = 0;
    while (zero_bin < 4096 && exp(-(double) zero_bin) > 0.0) zero_bin++;
    for (int b2 = 1; b2 <= zero_bin; b2++)
        if (!(exp(-(double) b2) < exp(-(double) (b2 - 1)))) {
            delete e;
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "exp() is not strictly monotone on the integers at %d", -b2);
        }
    pp.n_bins = zero_bin + 1;
    pp.thr_bin = -1;
    for (int b2 = 0; b2 < pp.n_bins; b2++) {
        const double post = std::min(1.0, exp(-(double) b2)); /* exactly 0.0 in the last bin */
        if (!(post < params->min_posterior_probability_for_partition)) pp.thr_bin = b2;
    }
    e->arrays.bind(&ctx->pool);
    {   /* what the last engine of this context left behind */
        std::lock_guard<std::mutex> lock(ctx->sibling_mu);
        e->spare.insert(e->spare.end(), ctx->spare_batches.begin(), ctx->spare_batches.end());
        ctx->spare_batches.clear();
        e->spare_levels.swap(ctx->spare_levels);
    }
    hipError_t he = e->leaf_part.alloc(4);
    if (he == hipSuccess) he = e->leaf_np.alloc(4);
    if (he == hipSuccess) he = e->leaf_count.alloc(4);
    if (he == hipSuccess) he = e->d_segs.alloc(mrp_engine::MAX_SEGS);
    const uint64_t lp[4] = {1, 0, 0, 0}; /* stRPHmm_construct hmm.c:97-133 */
    const uint32_t ln[4] = {0, 0, 0, 0};
    const int32_t lc[4] = {2, 0, 0, 0};  /* its single column has two cells */
    if (he == hipSuccess) he = hipMemcpy(e->leaf_part.p, lp, sizeof(lp), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->leaf_np.p, ln, sizeof(ln), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->leaf_count.p, lc, sizeof(lc), hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        mrp_engine_destroy(e);
        return mrp_set_error(MRP_ERR_HIP, "engine setup failed: %s", hipGetErrorString(he));
    }
    *out = e;
    return MRP_OK;
}

void mrp_engine_destroy(mrp_engine *e) {
    if (!e) return;
    mrp_context *ctx = e->ctx;
    if (getenv("MRP_TIMELINE") && !e->timeline.empty()) { /* one line per engine (= per concurrent batch of a call), times on the process clock */
        char buf[4096]; int o = snprintf(buf, sizeof(buf), "timeline: engine made at %.1f, ends at %.1f; levels (hmms @ launch):", fmod(e->t_created, 1e5), fmod(eng_now(), 1e5));
        for (auto &t : e->timeline) if (o < (int) sizeof(buf) - 40) o += snprintf(buf + o, sizeof(buf) - (size_t) o, " %lld@%.1f", t.first, fmod(t.second, 1e5));
        fprintf(stderr, "%s\n", buf);
    }
    if (getenv("MRP_TIMING")) {
        fprintf(stderr, "  levels: %.1f ms of the stream between the start of the layout kernels and the first kernel of the level proper, %.1f ms of it the host reacting to the totals (allocations, launches)\n", e->diag_layout_gap_ms, e->diag_react_ms);
        fprintf(stderr, "  context waits so far: %.1f ms wall, %.1f ms of thread CPU inside them\n", ctx->wait_wall_ms, ctx->wait_cpu_ms);
        ctx->wait_wall_ms = ctx->wait_cpu_ms = 0;
    }
    (void) hipSetDevice(ctx->device);
    (void) hipStreamSynchronize(ctx->stream);
    if (ctx->pre) (void) hipStreamSynchronize(ctx->pre);
    if (e->staged) { level_retire(e, e->staged); e->staged = nullptr; }
    for (auto *L : e->inflight) level_retire(e, L);
    e->inflight.clear();
    {   /* kept for the next engine of this context */
        std::lock_guard<std::mutex> lock(ctx->sibling_mu);
        for (auto *L : e->spare_levels) ctx->spare_levels.push_back(L);
        for (mrp_batch *b : e->spare) ctx->spare_batches.push_back(b);
    }
    e->spare_levels.clear();
    e->spare.clear();
    delete e;
    ctx->pool.reclaim();
}

}  /* extern "C" */

void mrp_engine_release_context_cache(mrp_context *ctx) {
    for (auto *L : ctx->spare_levels) delete L;
    ctx->spare_levels.clear();
    for (mrp_batch *b : ctx->spare_batches) mrp_batch_destroy(b);
    ctx->spare_batches.clear();
}

extern "C" {

int32_t mrp_engine_stride(const mrp_engine *e) { return e->pp.S; }

int mrp_engine_locate(const mrp_engine *e, int32_t seg, int64_t col0, const uint64_t **part, const uint32_t **np,
                      const int32_t **n_cells, const int32_t **n_merge) {
    if (!e || seg >= e->n_segs) return mrp_set_error(MRP_ERR_ARG, "mrp_engine_locate: no segment %d", seg);
    if (seg < 0) { *part = e->leaf_part.p; *np = e->leaf_np.p; *n_cells = e->leaf_count.p; *n_merge = nullptr; return MRP_OK; }
    const SegDev &sg = e->segtab[seg];
    *part = sg.part + col0 * e->pp.S; *np = sg.np + col0 * e->pp.S; *n_cells = sg.n_cells + col0; *n_merge = sg.n_merge + col0;
    return MRP_OK;
}

void mrp_engine_get_stats(const mrp_engine *e, mrp_engine_stats *out) { *out = e->stats; }

int mrp_engine_fetch(mrp_engine *e, void *dst, const void *src_dev, int64_t bytes) {
    if (bytes <= 0) return MRP_OK;
    ENG_TRY(hipSetDevice(e->ctx->device));
    ENG_TRY(hipMemcpyAsync(dst, src_dev, (size_t) bytes, hipMemcpyDeviceToHost, e->ctx->stream));
    return MRP_OK;
}

int mrp_engine_sync(mrp_engine *e) {
    ENG_TRY(hipSetDevice(e->ctx->device));
    ENG_TRY(e->ctx->wait_stream(e->ctx->stream));
    return MRP_OK;
}

}  /* extern "C" */

/* ---- stage: the static description of a level, built and uploaded while the level before runs ---- */
#define ENG_TRY_DUP(letter, expr) /* MRP_DUP names the kernel family: launched twice */ \
    do {                                                                                 \
        ENG_TRY(expr);                                                                   \
        if (mrp_dup(letter)) ENG_TRY(expr);                                              \
    } while (0)

static hipError_t eng_upload(void *dst, const void *src, size_t bytes, hipStream_t cs) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs) : hipSuccess;
}

/* step 1: a parked level object, or a new one */
static int level_take(mrp_engine *e, int64_t n, const mrp_xhmm *x, bool final_level, std::unique_ptr<mrp_engine_level_state> &L) {
    if (!e->spare_levels.empty()) {
        /* the parked level object whose page-locked staging block fits best: the levels of a call differ a hundredfold in size, and a
         * block that has to grow is freed and allocated again (milliseconds each, and both synchronize with the device) */
        size_t want = 4096 + (size_t) n * (sizeof(XDesc) + sizeof(PlanHmm) + sizeof(PruneHmm) + 12 + 4 * 64);
        for (int64_t i = 0; i < n; i++) want += 8 * (size_t) x[i].n_cols + sizeof(mrp_xpar) * (size_t) (x[i].n_a + x[i].n_b);
        size_t best = 0;
        long long best_score = -1;
        for (size_t q = 0; q < e->spare_levels.size(); q++) {
            const mrp_engine_level_state *c = e->spare_levels[q];
            long long score = c->stage.bytes >= want ? (long long) (c->stage.bytes - want) : (1ll << 40) + (long long) (want - c->stage.bytes);
            if (final_level != (c->frag.stage_block.bytes > 0)) score += 1ll << 36; /* (the final level alone stages the genome fragments' reads) */
            if (best_score < 0 || score < best_score) { best_score = score; best = q; }
        }
        L.reset(e->spare_levels[best]);
        e->spare_levels.erase(e->spare_levels.begin() + (long) best);
        return MRP_OK;
    }
    L.reset(new (std::nothrow) mrp_engine_level_state());
    if (!L) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    ENG_TRY(L->create_events());
    return MRP_OK;
}

/* step 2: the level's batch object; per hmm where its columns, reads, allele slots and parents start; chunk table; range checks
 * against the static bounds */
static int level_index(mrp_engine *e, mrp_engine_level_state *L, hipStream_t cs, bool *all_planes_out) {
    mrp_context *ctx = e->ctx;
    const int64_t n = L->n;
    const mrp_xhmm *x = L->x;
    if (e->spare.empty()) {
        mrp_batch *nb = nullptr;
        int rc = mrp_batch_create(ctx, &nb);
        if (rc != MRP_OK) return rc;
        L->b = nb;
    } else {
        L->b = e->spare.back();
        e->spare.pop_back();
    }
    mrp_batch *b = L->b;
    b->resident = true;
    HmmIndex &ix = L->ix;
    ix.col0.resize((size_t) n + 1); ix.read0.resize((size_t) n + 1); ix.slot0.resize((size_t) n + 1); ix.par0.resize((size_t) n + 1);
    ix.cost.resize((size_t) n); ix.chunk.resize((size_t) n);
    int64_t total_cols = 0, total_reads = 0, total_slots = 0, total_par = 0;
    bool all_planes = true;
    for (int64_t i = 0; i < n; i++) {
        const mrp_xhmm &h = x[i];
        if (h.n_cols < 1 || !h.col_start || !h.col_read_off || !h.chunk || h.n_a < 0 || h.n_b < 0 || (h.n_a + h.n_b > 0 && !h.par) ||
            h.ref_start < 0 || h.ref_end <= h.ref_start || h.ref_end > h.chunk->n_sites)
            return mrp_set_error(MRP_ERR_ARG, "mrp_engine_level: bad hmm %lld", (long long) i);
        const mrp_chunk *ch = h.chunk;
        if (ch->ctx->device != ctx->device) return mrp_set_error(MRP_ERR_ARG, "chunk missing or on a different device");
        int idx = -1;
        if (!b->chunks.empty() && b->chunks.back() == ch) idx = (int) b->chunks.size() - 1;
        for (size_t c = 0; idx < 0 && c < b->chunks.size(); c++)
            if (b->chunks[c] == ch) idx = (int) c;
        if (idx < 0) {
            idx = (int) b->chunks.size(); b->chunks.push_back(ch);
            /* a chunk still being uploaded (work queue): the level's structure kernel and, through L->uploaded, its other
             * kernels are ordered behind the end of the upload */
            if (ch->ready_pending.load()) {
                if (hipEventQuery(ch->ready) == hipSuccess) ch->ready_pending.store(false); /* over: never asked again */
                else ENG_TRY(hipStreamWaitEvent(cs, ch->ready, 0));
            }
        }
        ix.chunk[(size_t) i] = idx;
        const bool anc = (h.flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB) != 0;
        if (!anc) all_planes = false; /* (a column without the ancestor model needs bit planes only if its allele counts differ) */
        int64_t cb = 255ll * h.depth_sites;
        if (anc) cb += (2ll * ch->max_sub + ch->max_prior) * (int64_t) (h.ref_end - h.ref_start);
        ix.cost[(size_t) i] = cb;
        if ((anc && ch->max_alleles > MRP_MAX_ALLELES) || h.bound_max_cells > MRP_PRUNE_MAX_CELLS || h.bound_max_merge > MRP_PRUNE_MAX_CELLS ||
            h.bound_cells >= (1ll << 30) || cb >= (1ll << 30))
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "device-resident hmm %lld is outside the kernels' range", (long long) i);
        ix.col0[(size_t) i] = total_cols; ix.read0[(size_t) i] = total_reads; ix.slot0[(size_t) i] = total_slots; ix.par0[(size_t) i] = total_par;
        total_cols += h.n_cols;
        total_reads += h.n_col_reads; /* (= col_read_off[n_cols] and the allele slots of the interval, as the caller counted them: this loop */
        total_slots += h.n_slots;     /*  runs on the thread that feeds the device and stays inside the descriptions) */
        total_par += h.n_a + h.n_b;
    }
    ix.col0[(size_t) n] = total_cols;
    if (total_cols > 0x7FFFFFFFll) return mrp_set_error(MRP_ERR_UNSUPPORTED, "level with %lld columns", (long long) total_cols);
    ix.total_cols = total_cols; ix.total_reads = total_reads; ix.total_slots = total_slots; ix.total_par = total_par;
    *all_planes_out = all_planes;
    return MRP_OK;
}

/* step 3: the level's output -- the pruned hmms, fixed stride (the final level keeps one traced-back cell per column), and the
 * column structure the levels above will look up -- and the page-locked block of the uploads */
static int level_segment(mrp_engine *e, mrp_engine_level_state *L) {
    const int64_t total_cols = L->ix.total_cols;
    L->seg.reset(new (std::nothrow) Segment());
    if (!L->seg) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    Segment *seg = L->seg.get();
    seg->arrays.bind(&e->ctx->pool);
    ENG_TRY(seg->part.alloc((size_t) (total_cols * (L->final_level ? 1 : e->pp.S))));
    ENG_TRY(seg->np.alloc((size_t) (L->final_level ? 1 : total_cols * e->pp.S)));
    ENG_TRY(seg->n_cells.alloc((size_t) total_cols));
    ENG_TRY(seg->n_merge.alloc((size_t) total_cols));
    ENG_TRY(seg->cols.alloc((size_t) total_cols));
    ENG_TRY(seg->rbo.alloc((size_t) L->ix.total_reads));
    L->seg_id = e->n_segs++;
    SegDev &sd = e->segtab[L->seg_id];
    sd.part = seg->part.p; sd.np = seg->np.p; sd.n_cells = seg->n_cells.p; sd.n_merge = seg->n_merge.p; sd.cols = seg->cols.p; sd.rbo = seg->rbo.p;

    const std::vector<const mrp_chunk *> &chunks = L->b->chunks;
    ENG_TRY(L->stage.reserve(StageBlock(nullptr, (size_t) L->n, L->ix, chunks.size()).bytes));
    L->h = StageBlock(L->stage.p, (size_t) L->n, L->ix, chunks.size());
    for (size_t c = 0; c < chunks.size(); c++) L->h.chunks[c] = chunks[c]->dev;
    *L->h.seg = sd;
    return MRP_OK;
}

/* step 5: per hmm records and the 8 bytes per column the host contributes (parallel) */
static void level_records(mrp_engine *e, mrp_engine_level_state *L) {
    mrp_xhmm *x = L->x;
    const int64_t n = L->n, S = e->pp.S, out_stride = L->final_level ? 1 : S;
    const HmmIndex &ix = L->ix;
    const StageBlock &hb = L->h;
    const int32_t *pos = L->order.pos.data();
    Segment *seg = L->seg.get();
    const bool final_level = L->final_level;
    const int seg_id = L->seg_id;
    mrp_pool_set_tag(8); mrp_pool_set_weight(400); mrp_parallel_for(n, std::max<int64_t>(1, n / 256), [&](int64_t i) {
        mrp_xhmm &h = x[i];
        if (i + 3 < n) { __builtin_prefetch(x[i + 3].col_start); __builtin_prefetch(x[i + 3].col_read_off); __builtin_prefetch(x[i + 3].par); }
        const int K = h.n_cols;
        const int64_t colbase = ix.col0[(size_t) i];
        XDesc &d = hb.xd[i];
        d.col0 = colbase; d.read0 = ix.read0[(size_t) i]; d.slot0 = ix.slot0[(size_t) i]; d.par0 = ix.par0[(size_t) i];
        d.ref_start = h.ref_start; d.ref_end = h.ref_end; d.n_cols = K; d.n_a = h.n_a; d.n_b = h.n_b;
        d.chunk = ix.chunk[(size_t) i]; d.flags = h.flags; d.prune_pos = pos[i];
        if (h.n_a + h.n_b > 0) memcpy(hb.par + ix.par0[(size_t) i], h.par, sizeof(mrp_xpar) * (size_t) (h.n_a + h.n_b));
        memcpy(hb.cstart + colbase, h.col_start, sizeof(int32_t) * (size_t) K);
        memcpy(hb.croff + colbase, h.col_read_off, sizeof(int32_t) * (size_t) K);
        PlanHmm &p = hb.phmm[i];
        p.col0 = colbase; p.n_cols = K; p.flags = h.flags; p.cost_bound = ix.cost[(size_t) i];
        PruneHmm &q = hb.ph[pos[i]];
        q.col0 = colbase; q.n_cols = K; q.hmm_index = (int32_t) i;
        q.out_part = seg->part.p + colbase * out_stride;
        q.out_np = final_level ? seg->np.p : seg->np.p + colbase * S;
        q.out_n_cells = seg->n_cells.p + colbase;
        q.out_n_merge = seg->n_merge.p + colbase;
        h.seg = seg_id; h.col0 = colbase;
        h.err = 0;
    });
    mrp_pool_set_weight(0);
    hb.cstart[ix.total_cols] = 0;
}

/* step 4, second half: the launch classes go to the batch and the staging block, the level's maxima to its prune parameters */
static void level_plan(mrp_engine *e, mrp_engine_level_state *L) {
    mrp_context *ctx = e->ctx;
    mrp_batch *b = L->b;
    LevelOrder &o = L->order;
    level_classes(L->x, L->n, L->units, o);
    b->order_wide = o.wide.order; b->order_mid = o.mid.order; b->order_narrow = o.narrow.order;
    b->max_merge_wide = o.wide.max_merge; b->max_merge_mid = o.mid.max_merge; b->max_merge_narrow = o.narrow.max_merge;
    if (!o.wide.order.empty()) memcpy(L->h.ord_w, o.wide.order.data(), 4 * o.wide.order.size());
    if (!o.mid.order.empty()) memcpy(L->h.ord_m, o.mid.order.data(), 4 * o.mid.order.size());
    if (!o.narrow.order.empty()) memcpy(L->h.ord_n, o.narrow.order.data(), 4 * o.narrow.order.size());
    PruneParams &pp = L->pp;
    pp = e->pp;
    pp.max_cells = o.max_cells; pp.max_merge = o.max_merge;
    if (ctx->test_hooks & 8) pp.pairs = 0; /* test hook: the general prune chain, for A/B parity with the chain on complement pairs */
    if (L->units) pp.pairs = 2; /* (decided in level_stage: the level's arrays hold one entry per complement pair) */
    pp.pad = (ctx->test_hooks & 1) && e->stats.levels + (int64_t) e->inflight.size() == 1 ? 1 : 0; /* test hook, see mrp_context_set_test_hooks */
}

/* step 6: device side of the description + the descriptor arrays the structure and layout kernels fill */
static int level_describe(mrp_engine *e, mrp_engine_level_state *L, hipStream_t cs) {
    mrp_batch *b = L->b;
    const size_t n = (size_t) L->n, total_cols = (size_t) L->ix.total_cols, total_par = (size_t) L->ix.total_par;
    const StageBlock &hb = L->h;
    b->bind_pool(&e->ctx->pool);
    L->arrays.bind(&e->ctx->pool);
    ENG_TRY(L->d_plan.alloc(total_cols)); ENG_TRY(L->d_xd.alloc(n)); ENG_TRY(L->d_par.alloc(total_par));
    ENG_TRY(L->d_cstart.alloc(total_cols + 1)); ENG_TRY(L->d_croff.alloc(total_cols));
    ENG_TRY(L->d_phmm.alloc(n)); ENG_TRY(L->d_dims.alloc(4 * total_cols));
    ENG_TRY(L->d_tot.alloc(n)); ENG_TRY(L->d_base.alloc(n)); ENG_TRY(L->d_totals.alloc(8));
    ENG_TRY(L->d_tile_sums.alloc(6 * ((n + 255) / 256)));
    ENG_TRY(L->d_cc.alloc(total_cols)); ENG_TRY(L->d_ph.alloc(n)); ENG_TRY(L->d_col_hmm.alloc(total_cols));
    ENG_TRY(L->d_err.alloc(64)); ENG_TRY(L->d_err_hmm.alloc(n));
    ENG_TRY(b->d_hmms.alloc(n)); ENG_TRY(b->d_cols.alloc(total_cols)); ENG_TRY(b->d_scols.alloc(total_cols));
    ENG_TRY(b->d_pcols.alloc(total_cols)); ENG_TRY(b->d_tilecols.alloc(total_cols));
    ENG_TRY(b->d_chunks.alloc(b->chunks.size()));
    ENG_TRY(b->d_order_wide.alloc(b->order_wide.size())); ENG_TRY(b->d_order_mid.alloc(b->order_mid.size()));
    ENG_TRY(b->d_order_narrow.alloc(b->order_narrow.size())); ENG_TRY(b->d_order_f64.alloc(1));
    ENG_TRY(eng_upload(L->d_xd.p, hb.xd, sizeof(XDesc) * n, cs));
    ENG_TRY(eng_upload(L->d_par.p, hb.par, sizeof(mrp_xpar) * total_par, cs));
    ENG_TRY(eng_upload(L->d_cstart.p, hb.cstart, 4 * (total_cols + 1), cs));
    ENG_TRY(eng_upload(L->d_croff.p, hb.croff, 4 * total_cols, cs));
    ENG_TRY(eng_upload(L->d_phmm.p, hb.phmm, sizeof(PlanHmm) * n, cs));
    ENG_TRY(eng_upload(L->d_ph.p, hb.ph, sizeof(PruneHmm) * n, cs));
    ENG_TRY(eng_upload(b->d_order_wide.p, hb.ord_w, 4 * b->order_wide.size(), cs));
    ENG_TRY(eng_upload(b->d_order_mid.p, hb.ord_m, 4 * b->order_mid.size(), cs));
    ENG_TRY(eng_upload(b->d_order_narrow.p, hb.ord_n, 4 * b->order_narrow.size(), cs));
    ENG_TRY(eng_upload(b->d_chunks.p, hb.chunks, sizeof(DevChunk) * b->chunks.size(), cs));
    ENG_TRY(eng_upload(e->d_segs.p + L->seg_id, hb.seg, sizeof(SegDev), cs));
    ENG_TRY(hipMemsetAsync(L->d_err.p, 0, 256, cs));
    ENG_TRY(hipMemsetAsync(L->d_err_hmm.p, 0, sizeof(int32_t) * n, cs));
    return MRP_OK;
}

/* step 7: the columns of the level, one thread each: parents, connectors, reads, allele slots (also on the copy stream: the
 * tables it reads were written by the structure kernels of the levels below, on the same stream) */
static int level_structure(mrp_engine *e, mrp_engine_level_state *L, hipStream_t cs) {
    StructureIn si{};
    si.xd = L->d_xd.p; si.n_hmms = L->n; si.n_cols = L->ix.total_cols; si.par = L->d_par.p; si.col_start = L->d_cstart.p; si.col_roff = L->d_croff.p;
    si.segs = e->d_segs.p; si.chunks = L->b->d_chunks.p;
    si.leaf_part = e->leaf_part.p; si.leaf_np = e->leaf_np.p; si.leaf_count = e->leaf_count.p;
    si.stride = e->pp.S; si.fused = L->fused ? 1 : 0;
    si.plan = L->d_plan.p; si.cols = L->seg->cols.p; si.rbo = L->seg->rbo.p; si.col_hmm = L->d_col_hmm.p;
    si.err = L->d_err.p; si.err_hmm = L->d_err_hmm.p;
    ENG_TRY_DUP('t', mrp_launch_structure(si, cs));
    return MRP_OK;
}

/* step 8: genome fragments on the device, if every hmm of the stage brings its chunk's reads */
int FragStage::stage(const mrp_xhmm *x, int64_t n, const std::vector<int32_t> &perm, const HmmIndex &ix, DevPool *pl, hipStream_t cs) {
    on = false;
    bool all = true;
    for (int64_t i = 0; i < n && all; i++) all = x[i].frag_reads && x[i].frag_by_pool && x[i].frag_sites && x[i].frag_reads1 && x[i].frag_reads2 && x[i].frag_n_reads > 0;
    if (!all) return MRP_OK;
    hmms.resize((size_t) n);
    int64_t r0 = 0, d0 = 0, s0 = 0, l0 = 0;
    for (int64_t i = 0; i < n; i++) {
        const mrp_xhmm &h = x[(size_t) perm[(size_t) i]];
        FragHmm &f = hmms[(size_t) i];
        f.reads0 = r0; f.disc0 = d0; f.site0 = s0; f.list0 = l0; f.slot0 = ix.read0[(size_t) perm[(size_t) i]];
        f.n_reads = h.frag_n_reads; f.n_discarded = h.frag_n_discarded; f.ref_start = h.ref_start; f.length = h.ref_end - h.ref_start;
        f.max_iterations = h.frag_iterations; f.pad = 0;
        r0 += h.frag_n_reads; d0 += h.frag_n_discarded; s0 += f.length; l0 += 2 * (int64_t) h.frag_n_reads + 2;
    }
    sites_total = s0; list_total = l0;
    FragHmm *fh = nullptr; FragRead *fr = nullptr; int32_t *fp = nullptr, *fd = nullptr;
    auto carve_in = [&](void *block) {
        BlockCarver c(block);
        fh = c.take<FragHmm>((size_t) n); fr = c.take<FragRead>((size_t) r0); fp = c.take<int32_t>((size_t) r0); fd = c.take<int32_t>((size_t) d0 + 1);
        return c.used;
    };
    auto carve_out = [&](void *block) {
        BlockCarver c(block);
        h_sites = c.take<FragSite>((size_t) s0); h_lists = c.take<int32_t>(2 * (size_t) l0); h_counts = c.take<int32_t>(2 * (size_t) n);
        return c.used;
    };
    ENG_TRY(stage_block.reserve(carve_in(nullptr)));
    carve_in(stage_block.p);
    memcpy(fh, hmms.data(), sizeof(FragHmm) * (size_t) n);
    mrp_parallel_for(n, 1, [&](int64_t i) {
        const mrp_xhmm &h = x[(size_t) perm[(size_t) i]];
        const FragHmm &f = hmms[(size_t) i];
        for (int32_t r = 0; r < h.frag_n_reads; r++) {
            FragRead &q = fr[f.reads0 + r];
            q.ref_start = h.frag_reads[r].ref_start; q.length = h.frag_reads[r].length; q.pool_offset = h.frag_reads[r].pool_offset;
        }
        memcpy(fp + f.reads0, h.frag_by_pool, 4 * (size_t) h.frag_n_reads);
        if (h.frag_n_discarded > 0) memcpy(fd + f.disc0, h.frag_discarded, 4 * (size_t) h.frag_n_discarded);
    });
    arrays.bind(pl);
    ENG_TRY(d_hmms.alloc((size_t) n)); ENG_TRY(d_reads.alloc((size_t) r0)); ENG_TRY(d_by_pool.alloc((size_t) r0));
    ENG_TRY(d_disc.alloc((size_t) d0 + 1)); ENG_TRY(d_lists.alloc(2 * (size_t) l0)); ENG_TRY(d_work.alloc(2 * (size_t) l0));
    ENG_TRY(d_counts.alloc(2 * (size_t) n)); ENG_TRY(d_col_read.alloc((size_t) ix.total_reads + 1)); ENG_TRY(d_col_cnt.alloc(2 * (size_t) ix.total_cols));
    ENG_TRY(d_sites.alloc((size_t) s0)); ENG_TRY(d_col_part.alloc((size_t) ix.total_cols)); ENG_TRY(d_read_key.alloc(2 * (size_t) r0));
    ENG_TRY(eng_upload(d_hmms.p, fh, sizeof(FragHmm) * (size_t) n, cs));
    ENG_TRY(eng_upload(d_reads.p, fr, sizeof(FragRead) * (size_t) r0, cs));
    ENG_TRY(eng_upload(d_by_pool.p, fp, 4 * (size_t) r0, cs));
    ENG_TRY(eng_upload(d_disc.p, fd, 4 * (size_t) d0, cs));
    ENG_TRY(results.reserve(carve_out(nullptr)));
    carve_out(results.p);
    on = true;
    return MRP_OK;
}

int FragStage::fetch(int64_t n, hipStream_t s) {
    ENG_TRY(hipMemcpyAsync(h_sites, d_sites.p, sizeof(FragSite) * (size_t) sites_total, hipMemcpyDeviceToHost, s));
    ENG_TRY(hipMemcpyAsync(h_lists, d_lists.p, 8 * (size_t) list_total, hipMemcpyDeviceToHost, s));
    ENG_TRY(hipMemcpyAsync(h_counts, d_counts.p, 8 * (size_t) n, hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

void FragStage::scatter(mrp_xhmm *x, int64_t n, const std::vector<int32_t> &perm, const int32_t *err_hmm) const {
    mrp_parallel_for(n, 1, [&](int64_t j) {
        mrp_xhmm &h = x[(size_t) perm[(size_t) j]];
        const FragHmm &f = hmms[(size_t) j];
        h.frag_done = 0;
        if (err_hmm[j] != 0) return;
        const int cap = 2 * f.n_reads + 2;
        const int n1 = h_counts[2 * j], n2 = h_counts[2 * j + 1];
        if (n1 < 0 || n2 < 0 || n1 > cap || n2 > cap) return;
        memcpy(h.frag_sites, h_sites + f.site0, sizeof(FragSite) * (size_t) f.length);
        memcpy(h.frag_reads1, h_lists + 2 * f.list0, 4 * (size_t) n1);
        memcpy(h.frag_reads2, h_lists + 2 * f.list0 + cap, 4 * (size_t) n2);
        h.frag_n1 = n1; h.frag_n2 = n2; h.frag_done = 1;
    });
}

static int level_stage(mrp_engine *e, int64_t n, mrp_xhmm *x, bool final_level) {
    if (!e || n < 0 || (n > 0 && !x)) return mrp_set_error(MRP_ERR_ARG, "mrp_engine_level: bad arguments");
    if (e->staged) return mrp_set_error(MRP_ERR_ARG, "mrp_engine_level_stage: a staged level was not launched");
    if (n == 0) return MRP_OK;
    mrp_context *ctx = e->ctx;
    ENG_TRY(hipSetDevice(ctx->device));
    hipStream_t cs = nullptr; /* copy stream: nothing here depends on the kernels in flight */
    ENG_TRY(ctx->copy_stream(&cs));
    if (e->n_segs >= mrp_engine::MAX_SEGS) return mrp_set_error(MRP_ERR_UNSUPPORTED, "more than %d levels", mrp_engine::MAX_SEGS);
    std::unique_ptr<mrp_engine_level_state> L;
    int rc = level_take(e, n, x, final_level, L);
    if (rc != MRP_OK) return rc;
    L->t.begin = eng_now();
    L->x = x;
    L->n = n;
    L->final_level = final_level;
    L->fused = !final_level && !(ctx->test_hooks & 2);
    for (int64_t i = 0; i < n && L->fused; i++)
        if (x[i].flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB) L->fused = false;
    /* one array entry per complement pair (MRP_XF_UNITS) where the one-pass cross product + emission kernel writes the level and
     * the prune reads it by units; test hook bit 4 keeps one entry per cell.  (test hook bit 3: the general prune chain) */
    L->units = L->fused && e->pp.pairs != 0 && !(ctx->test_hooks & (8 | 16));

    double tm[5];
    bool all_planes = true;
    tm[0] = eng_now();
    if ((rc = level_index(e, L.get(), cs, &all_planes)) != MRP_OK) return rc;
    tm[1] = eng_now();
    if ((rc = level_segment(e, L.get())) != MRP_OK) return rc;
    tm[2] = eng_now();
    level_sort(x, n, L->units, L->order);
    level_records(e, L.get());
    tm[3] = eng_now();
    level_plan(e, L.get());
    tm[4] = eng_now();
    if ((rc = level_describe(e, L.get(), cs)) != MRP_OK) return rc;
    if ((rc = level_structure(e, L.get(), cs)) != MRP_OK) return rc;
    L->frag.on = false;
    if (final_level && (rc = L->frag.stage(x, n, L->order.perm, L->ix, &ctx->pool, cs)) != MRP_OK) return rc;
    ENG_TRY(hipEventRecord(L->uploaded, cs));
    /* which of the two packing kernels has columns to look at (they filter by PlaneCol.need_planes) */
    L->any_pack = !all_planes;
    L->any_planes = !L->fused;
    /* results come back into a second page-locked block */
    ENG_TRY(L->results.reserve(ResultsBlock(nullptr, (size_t) n, (size_t) L->ix.total_cols, final_level).bytes));
    L->res = ResultsBlock(L->results.p, (size_t) n, (size_t) L->ix.total_cols, final_level);
    L->b->stats.n_hmms = n;
    L->b->stats.n_columns = L->ix.total_cols;
    L->t.staged = eng_now();
    if (getenv("MRP_TIMING"))
        fprintf(stderr, "      stage: offsets+chunks %.2f ms, segment+staging %.2f, records %.2f, classes %.2f, allocs+uploads %.2f\n", tm[1] - tm[0],
                tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], L->t.staged - tm[4]);
    e->staged = L.release();
    return MRP_OK;
}

/* ---- end: the per-hmm error flags of the running level (and the final level's results) ---- */
/* Per hmm: a parent outside the closed-form cross product's pair order, or a merge cell the kept cells lead to that
 * hmm.c:1090-1100 would drop, means "not handled on the device": the caller redoes that hmm's chunk on the hashing path
 * (whatever else the kernels flagged for it came from the discarded arrays).  Posterior / range violations on an hmm
 * that is otherwise fine are the reference's st_errAbort cases. */
static int level_scatter_errors(mrp_engine_level_state *Lp) {
    int rc = MRP_OK;
    if (Lp->res.err[0] == 0) return rc;
    for (int64_t j = 0; j < Lp->n && rc == MRP_OK; j++) {
        const int32_t bits = Lp->res.err_hmm[j];
        if (bits == 0) continue;
        mrp_xhmm &xq = Lp->x[(size_t) Lp->order.perm[(size_t) j]];
        xq.err = bits;
        if (bits & (MRP_ENGINE_ERR_STRUCTURE | MRP_ENGINE_ERR_MERGE)) {
            /* the chunk leaves the resident path: said at once (the caller says the same when it settles the level), so that the
             * levels in flight behind this one -- they ran on this hmm's discarded arrays -- are not held to what they raise */
            if (xq.discarded) *const_cast<int *>(xq.discarded) = 1;
            continue;
        }
        /* an hmm whose chunk already left the resident path at the level before (this level was staged before that was
         * known): it ran on a discarded parent's arrays, whatever it raised is that parent's */
        if (xq.discarded && *xq.discarded) continue;
        if (bits & MRP_ENGINE_ERR_POSTERIOR) rc = mrp_set_error(MRP_ERR_ARG, "ERROR: invalid prob (f + b exceeds the column total)");
        else rc = mrp_set_error(MRP_ERR_LOOKUP, "device-resident merge: transition index out of range");
    }
    return rc;
}

/* the final level's traced-back paths, sweep totals and genome fragments go to the caller's arrays */
static void level_scatter_final(mrp_engine_level_state *Lp) {
    int64_t colbase = 0;
    for (int64_t i = 0; i < Lp->n; i++) {
        mrp_xhmm &h = Lp->x[i];
        if (h.n_cells) memcpy(h.n_cells, Lp->res.path_cell + colbase, sizeof(int32_t) * (size_t) h.n_cols);
        if (h.path_part) memcpy(h.path_part, Lp->res.path_part + colbase, sizeof(uint64_t) * (size_t) h.n_cols);
        h.hmm_forward = Lp->res.fb[(size_t) (2 * i)];
        h.hmm_backward = Lp->res.fb[(size_t) (2 * i + 1)];
        colbase += h.n_cols;
    }
    if (Lp->frag.on) Lp->frag.scatter(Lp->x, Lp->n, Lp->order.perm, Lp->res.err_hmm);
}

static void level_book_stats(mrp_engine *e, mrp_engine_level_state *Lp) {
    float t_cross = 0, t_sweep = 0, t_prune = 0;
    (void) hipEventElapsedTime(&t_cross, Lp->ev[0], Lp->ev[1]);
    (void) hipEventElapsedTime(&t_sweep, Lp->ev[1], Lp->ev[2]);
    (void) hipEventElapsedTime(&t_prune, Lp->ev[2], Lp->ev[3]);
    e->stats.levels += 1;
    e->stats.hmms += Lp->n;
    e->stats.columns += Lp->ix.total_cols;
    e->stats.cells += Lp->res.totals[4];       /* the cross products' cells / merge cells (the arrays may hold units, mrp_engine.h) */
    e->stats.merge_cells += Lp->res.totals[5];
    e->stats.cross_ms += t_cross;
    e->stats.sweep_ms += t_sweep;
    e->stats.prune_ms += t_prune;
    e->stats.device_ms += t_cross + t_sweep + t_prune;
    {   /* (diagnostics, MRP_TIMING) the stream between the layout kernels' start and the level's first own kernel: layout kernels,
         * totals back, the host's reaction (allocations, launches) */
        float t_lay = 0;
        (void) hipEventElapsedTime(&t_lay, Lp->lay0, Lp->ev[0]);
        e->diag_layout_gap_ms += t_lay; e->diag_react_ms += Lp->t.react_ms > 0 ? Lp->t.react_ms : 0;
    }
    {   /* by kernel family: packing, cross product + emission, recursion (the batch's own events), prune, compaction */
        float t_pack = 0, t_emit = 0, t_rec = 0, t_pr = 0;
        mrp_batch_last_launch_ms(Lp->b, &t_pack, &t_emit, &t_rec);
        if (!Lp->final_level) (void) hipEventElapsedTime(&t_pr, Lp->ev[2], Lp->ev[4]);
        e->stats.pack_ms += t_pack;
        e->stats.cross_emit_ms += t_cross + t_emit;
        e->stats.recursion_ms += t_rec;
        e->stats.prune_kernel_ms += Lp->final_level ? 0.0 : t_pr;
        e->stats.compact_ms += Lp->final_level ? t_prune : t_prune - t_pr; /* (final level: the trace back) */
    }
}

/* one level whose `done` event is complete (or whose stream has been waited for) */
static int level_finish_one(mrp_engine *e, mrp_engine_level_state *Lp, bool complete) {
    if (getenv("MRP_TIMING")) {
        fprintf(stderr, "  level: %lld hmms %lld cols %lld cells: staged in %.1f ms, launch (layout + totals + queue) %.1f ms  [stage began at %.1f ms, launched at %.1f ms on the process clock]\n", (long long) Lp->n,
                (long long) Lp->ix.total_cols, (long long) Lp->res.totals[0], Lp->t.staged - Lp->t.begin, Lp->t.launch_ms, fmod(Lp->t.begin, 1e5), fmod(Lp->t.launched, 1e5));
#if defined(PRUNE_EXP_CLOCK) || defined(PRUNE_EXP_CLOCK2) || defined(XE_CLOCK)
        fprintf(stderr, "  prune clocks (first hmm; shader cycles):");
        for (int i = 0; i < 12; i++) fprintf(stderr, " %llu", Lp->clk[i]);
        fprintf(stderr, "\n");
#endif
    }
    const int rc = level_scatter_errors(Lp);
    if (rc == MRP_OK) {
        if (Lp->final_level) level_scatter_final(Lp);
        level_book_stats(e, Lp);
        e->segments.push_back(std::move(Lp->seg));
    }
    e->n_ended++;
    level_retire(e, Lp, complete);
    return rc;
}

/* ends every level in flight, oldest first, after ONE wait for the stream they were queued on */
static int level_finish(mrp_engine *e) {
    if (e->inflight.empty()) return MRP_OK;
    mrp_context *ctx = e->ctx;
    int rc = MRP_OK;
    hipError_t se = hipSetDevice(ctx->device);
    if (se == hipSuccess) se = ctx->wait_stream(ctx->stream);
    if (se != hipSuccess) rc = mrp_set_error(MRP_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(se));
    std::vector<mrp_engine_level_state *> all;
    all.swap(e->inflight);
    for (auto *Lp : all) {
        if (rc == MRP_OK) rc = level_finish_one(e, Lp, false);
        else { e->n_ended++; level_retire(e, Lp); }
    }
    return rc;
}

/* ends the levels in flight whose work is over (oldest first, as far as their events say so); never waits */
static int level_finish_ready(mrp_engine *e) {
    int rc = MRP_OK;
    while (rc == MRP_OK && !e->inflight.empty()) {
        mrp_engine_level_state *Lp = e->inflight.front();
        if (!Lp->done || hipEventQuery(Lp->done) != hipSuccess) { (void) hipGetLastError(); break; }
        e->inflight.erase(e->inflight.begin());
        rc = level_finish_one(e, Lp, true);
    }
    return rc;
}

/* ---- launch: layout on the device, four totals back, allocation, the level's kernels ---- */
/* step 1: the layout kernels behind the uploads, and the copy of their totals */
static int launch_layout(mrp_engine *e, mrp_engine_level_state *L, hipStream_t s) {
    mrp_batch *b = L->b;
    LayoutOut lo{};
    lo.dims = L->d_dims.p; lo.tot = L->d_tot.p; lo.base = L->d_base.p; lo.totals = L->d_totals.p; lo.tile_sums = L->d_tile_sums.p;
    lo.hmms = b->d_hmms.p; lo.cols = b->d_cols.p; lo.scols = b->d_scols.p; lo.pcols = b->d_pcols.p; lo.tilecols = b->d_tilecols.p;
    lo.ccols = L->d_cc.p;
    ENG_TRY(hipStreamWaitEvent(s, L->uploaded, 0));
    ENG_TRY(hipEventRecord(L->lay0, s));
    ENG_TRY_DUP('l', mrp_launch_layout(L->d_plan.p, L->d_phmm.p, L->n, L->ix.total_cols, b->d_chunks.p, e->pp.S,
                                       (e->params.include_inverted_partitions ? MRP_XF_INVERTED : 0u) | (L->units ? MRP_XF_UNITS : 0u), lo, s));
    ENG_TRY(hipMemcpyAsync(L->res.totals, L->d_totals.p, 48, hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

/* step 2.  Deferred launch (round 5): a small merge level -- its arrays at most DEFER_BYTES (1 GB) by the hmms' STATIC bounds, four
 * times that and at most DEFER_LEVELS levels in flight -- does not wait for its totals: the arrays are sized by the bounds (the
 * layout kernels' offsets stay inside them: every count is clamped to what the bounds assume), its kernels are queued behind
 * the layout kernels at once and the level before is ended whenever its event has completed.  A call of one chunk walks eleven levels whose kernels take a
 * millisecond or two each: the wait (totals back, the host awake again, two dozen allocations, a dozen launches) left the device
 * idle for a third of a millisecond per level.  The large levels keep the wait: bounds are loose there (a pruned column of 100
 * cells times another is the bound, a fifth of it the average) and their arrays are what the device's memory goes to.
 * Test hook bit 5: no level is deferred. */
static constexpr int64_t DEFER_BYTES = (int64_t) 1024 << 20;
static constexpr size_t DEFER_LEVELS = 12;
static bool level_defers(const mrp_engine *e, const mrp_engine_level_state *L) {
    const int64_t bound_bytes = level_bound_bytes(L);
    return !(e->ctx->test_hooks & 32) && L->fused && !L->final_level && bound_bytes <= DEFER_BYTES &&
           e->inflight_bytes + bound_bytes <= 4 * DEFER_BYTES && e->inflight.size() < DEFER_LEVELS;
}

/* steps 3 and 4: the batch's cell arrays, sized by the totals (or the bounds), and the device view of the batch */
static int launch_size_batch(mrp_engine_level_state *L, int64_t cells, int64_t merge, int64_t tiles_fast, int64_t tiles) {
    mrp_batch *b = L->b;
    const int64_t n = L->n, total_cols = L->ix.total_cols, n_slots = L->ix.total_slots;
    b->n_cells_total = cells; b->n_merge = merge; b->n_slots = n_slots; b->n_tiles_dev = tiles; b->n_fast_tiles = tiles_fast;
    b->stats.n_cells = cells; b->stats.n_merge_cells = merge;
    b->stats.algorithmic_bytes = 24 * cells + 32 * merge + 8 * total_cols;
    const size_t nC = (size_t) cells;
    if (L->fused) { b->d_partition.release(); b->n_tiles_dev = 0; b->n_fast_tiles = 0; }
    else ENG_TRY(b->d_partition.alloc(nC));
    ENG_TRY(b->d_np.alloc(nC)); ENG_TRY(b->d_cost.alloc(nC));
    ENG_TRY(b->d_f32.alloc(nC)); ENG_TRY(b->d_b32.alloc(nC));
    ENG_TRY(b->d_mf32.alloc((size_t) merge)); ENG_TRY(b->d_mb32.alloc((size_t) merge));
    if (!L->fused) ENG_TRY(b->d_tiles.alloc((size_t) tiles));
    ENG_TRY(b->d_planes.alloc((size_t) n_slots * 8)); ENG_TRY(b->d_slot_total.alloc((size_t) n_slots));
    ENG_TRY(b->d_slot_bytes.alloc((size_t) n_slots * 16));
    ENG_TRY(b->d_total.alloc((size_t) total_cols)); ENG_TRY(b->d_hmm_fb.alloc(2 * (size_t) n));
    MrpBatchDev &d = b->dev;
    d = b->view(); /* (the fp64 arrays, the wide transitions and the lists were never allocated: NULL) */
    d.read_byte_off = L->seg->rbo.p;
    d.pack_list = nullptr; d.plane_list = nullptr; d.list_filter = 1; /* every column, filtered by PlaneCol.need_planes */
    d.n_pack_list = L->any_pack ? total_cols : 0; d.n_plane_list = L->any_planes ? total_cols : 0;
    d.n_hmms = n; d.n_cols = total_cols; d.n_cells = cells; d.n_merge = merge; d.n_slots = n_slots;
    b->uploaded = true;
    b->outs.clear(); /* device-only */
    return MRP_OK;
}

/* step 5: cross product, the batch's sweeps, then trace back (+ fragments) or one-wave kernel, prune and compaction */
static int launch_kernels(mrp_engine *e, mrp_engine_level_state *L, hipStream_t s) {
    mrp_batch *b = L->b;
    const int64_t n = L->n, total_cols = L->ix.total_cols;
    const size_t kept = L->final_level ? 0 : (size_t) total_cols * (size_t) e->pp.S;
    LaunchCensus *const census = &e->ctx->census;
    if (!L->final_level) {
        ENG_TRY(L->d_kept.alloc(kept)); ENG_TRY(L->d_keptm.alloc(kept)); ENG_TRY(L->d_kept_np.alloc(kept));
        ENG_TRY(L->d_nkept.alloc((size_t) total_cols)); ENG_TRY(L->d_nkeptm.alloc((size_t) total_cols));
    }
    PruneScratch sc{};
    sc.kept = L->d_kept.p; sc.kept_np = L->d_kept_np.p; sc.keptm = L->d_keptm.p; sc.n_kept = L->d_nkept.p; sc.n_keptm = L->d_nkeptm.p;
    sc.err = L->d_err.p;
    sc.err_hmm = L->d_err_hmm.p;
    if (L->fused) {
        /* the packed profile bytes first (mrp_batch_launch), then cross product + emission in one pass; no tiles, no
         * partitions, the batch's own emission launch finds nothing to do */
        ENG_TRY(hipEventRecord(L->ev[0], s));
        ENG_TRY(hipEventRecord(L->ev[1], s));
        b->pre_sweep = [L, census](hipStream_t st) -> hipError_t {
            return mrp_launch_cross_emit(L->d_cc.p, L->b->dev, L->d_err.p, L->d_col_hmm.p, L->d_err_hmm.p, L->pp.max_cells, 2 * L->order.n_mini > L->n, st, census);
        };
    } else {
        b->pre_sweep = nullptr;
        ENG_TRY(mrp_launch_tiles(b->d_cols.p, b->d_tilecols.p, total_cols, b->d_tiles.p, s));
        ENG_TRY(hipEventRecord(L->ev[0], s));
        ENG_TRY(mrp_launch_cross(L->d_cc.p, total_cols, b->d_partition.p, b->d_np.p, L->d_err.p, L->d_col_hmm.p, L->d_err_hmm.p, s, census));
        ENG_TRY(hipEventRecord(L->ev[1], s));
    }
    const int rc = mrp_batch_launch(b);
    b->pre_sweep = nullptr;
    if (rc != MRP_OK) return rc;
    ENG_TRY(hipEventRecord(L->ev[2], s));
    if (L->final_level) {
        ENG_TRY_DUP('b', mrp_launch_traceback(b->dev, L->d_ph.p, n, L->d_err.p, L->d_err_hmm.p, s, census));
        if (L->frag.on) ENG_TRY(mrp_launch_fragments(b->dev, L->d_ph.p, n, L->frag.device_arrays(), L->d_err.p, L->d_err_hmm.p, s, census));
    } else {
        const int64_t n_mini = L->order.n_mini, n_reg = n - n_mini;
        ENG_TRY_DUP('m', mrp_launch_mini(b->dev, L->d_cc.p, L->d_ph.p + n_reg, n_mini, n_reg, L->pp, sc, s, census));
        ENG_TRY_DUP('r', mrp_launch_prune(b->dev, L->d_cc.p, L->d_ph.p, n_reg, L->pp, sc, s, census));
        ENG_TRY(hipEventRecord(L->ev[4], s));
        ENG_TRY_DUP('c', mrp_launch_compact(b->dev, L->d_cc.p, L->d_ph.p, L->d_col_hmm.p, total_cols, n_reg, L->pp, sc, s, census));
    }
    ENG_TRY(hipEventRecord(L->ev[3], s));
    return MRP_OK;
}

/* step 6: the error flags and, at the final level, the paths, sweep totals and fragments come back; `done` behind them */
static int launch_fetch_results(mrp_engine_level_state *L, hipStream_t s) {
    const int64_t n = L->n, total_cols = L->ix.total_cols;
    if (L->final_level) {
        ENG_TRY(hipMemcpyAsync(L->res.path_cell, L->seg->n_cells.p, sizeof(int32_t) * (size_t) total_cols, hipMemcpyDeviceToHost, s));
        ENG_TRY(hipMemcpyAsync(L->res.path_part, L->seg->part.p, sizeof(uint64_t) * (size_t) total_cols, hipMemcpyDeviceToHost, s));
        ENG_TRY(hipMemcpyAsync(L->res.fb, L->b->dev.hmm_fb, sizeof(double) * (size_t) (2 * n), hipMemcpyDeviceToHost, s));
        if (L->frag.on) { const int rc = L->frag.fetch(n, s); if (rc != MRP_OK) return rc; }
    }
    ENG_TRY(hipMemcpyAsync(L->res.err, L->d_err.p, 16, hipMemcpyDeviceToHost, s));
    ENG_TRY(hipMemcpyAsync(L->res.err_hmm, L->d_err_hmm.p, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, s));
#if defined(PRUNE_EXP_CLOCK) || defined(PRUNE_EXP_CLOCK2) || defined(XE_CLOCK)
    ENG_TRY(hipMemcpyAsync(L->clk, L->d_err.p + 4, 96, hipMemcpyDeviceToHost, s));
#endif
    ENG_TRY(hipEventRecord(L->done, s));
    return MRP_OK;
}

static int level_launch_impl(mrp_engine *e, mrp_engine_level_state *L) {
    mrp_context *ctx = e->ctx;
    ENG_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const double t0 = eng_now();
    int rc = launch_layout(e, L, s);
    if (rc != MRP_OK) return rc;
    int64_t cells, merge, tiles_fast = 0, tiles = 0;
    if (level_defers(e, L)) {
        if ((rc = level_finish_ready(e)) != MRP_OK) return rc;
        cells = L->order.bound_cells; merge = L->order.bound_merge;
        L->deferred = true;
        e->inflight_bytes += level_bound_bytes(L);
    } else {
        /* the one host wait of a level: it also ends the levels before (their error flags are in) */
        if ((rc = level_finish(e)) != MRP_OK) return rc;
        ENG_TRY(ctx->wait_stream(s));
        L->t.react_ms = -eng_now();
        ctx->pool.reclaim(); /* the blocks of the level before can be reused */
        const int64_t *tot = L->res.totals;
        cells = tot[0]; merge = tot[1]; tiles_fast = tot[2]; tiles = tot[2] + tot[3];
    }
    if ((rc = launch_size_batch(L, cells, merge, tiles_fast, tiles)) != MRP_OK) return rc;
    if ((rc = launch_kernels(e, L, s)) != MRP_OK) return rc;
    if ((rc = launch_fetch_results(L, s)) != MRP_OK) return rc;
    if (L->t.react_ms < 0) L->t.react_ms += eng_now();
    L->t.launched = eng_now();
    if (getenv("MRP_TIMELINE")) e->timeline.emplace_back((long long) L->n, L->t.launched);
    L->t.launch_ms = L->t.launched - t0;
    return MRP_OK;
}

static int level_launch(mrp_engine *e) {
    if (!e->staged) return level_finish(e); /* an empty level still ends the ones before */
    mrp_engine_level_state *L = e->staged;
    e->staged = nullptr;
    int rc = level_launch_impl(e, L);
    if (rc != MRP_OK) { level_retire(e, L); return rc; }
    e->inflight.push_back(L);
    return MRP_OK;
}

extern "C" {

int mrp_engine_level_stage(mrp_engine *e, int64_t n, mrp_xhmm *x) { return level_stage(e, n, x, false); }
int mrp_engine_final_stage(mrp_engine *e, int64_t n, mrp_xhmm *x) { return level_stage(e, n, x, true); }
int mrp_engine_level_launch(mrp_engine *e) { return level_launch(e); }
int mrp_engine_level_end(mrp_engine *e) {
    if (!e) return mrp_set_error(MRP_ERR_ARG, "mrp_engine_level_end: NULL engine");
    return level_finish(e);
}
int64_t mrp_engine_levels_ended(const mrp_engine *e) { return e ? e->n_ended : 0; }

}  /* extern "C" */
